"""Test helper (not a conftest): the light side of the path estimator -- the point sampled on an emitter, the emitter pdf, the distant-light
direction, the one-sample light / BSDF mixture and the direct-light pass's steps 3 to 7 on Lambert surfaces -- in numpy and float64, with no
device and no oracle.  Written from the specification: the reference project's surface_sample.rs:69-117, rand.rs, math.rs:8-20, light.rs:52-55,
lib.rs:225-342 and 959-1066, the header's statement of the direct-light pass (include/rene_hip.h, "The sample of pixel (px, py)") and the quirk
list of SURVEY.md section 8 a.  Quirks kept: Q1 (the integrator asks pdf(wi, normal)), Q4 (a sphere emitter's cone from the mean absolute
diagonal of object_to_world), Q5 (pdf_l over emit_object_len, the emitter structure queried along wi whichever branch drew it), Q6 (`u32 %
prim_count`), and wi = normalize((p + dir) - p) of a distant light, which cancels in fp32 by design.

Inputs are exact: the fp32 numbers the ABI carries (vertices, matrices, colours, light directions), the rays, and the random numbers out of
bsdf_reference's restatement of PCG32si.  What the packer computes from them on the host -- world-space vertices, the unit normal and the
area of an emitter triangle -- is NOT taken from the packer: the reference forms them in float64 from the ABI's numbers and budgets the
packer's fp32 arithmetic, so a table that holds a neighbouring float is outside the allowance like any other wrong number.

THE ALLOWANCE.  u = 2^-24 (half an fp32 ulp: one correctly rounded operation).  As bsdf_reference.py and medium_reference.py assume:
v_rcp_f32, v_rsq_f32, v_sqrt_f32 at 1 ulp (2 u), qdiv (v_rcp_f32 and a product) at 2 ulp (4 u), `/` by a constant at 2.5 ulp (5 u:
-fno-hip-fp32-correctly-rounded-divide-sqrt), a sum of k products at k u of the sum of their magnitudes.  Every constant below is written
next to its count.  A quantity whose conditioning varies carries the condition in the formula, not in the constant:

  emitter point, triangle   u (N_COMBINE sum_k |p_k b_k| + N_XFORM sum_k b_k sum_j |v_kj m_j|): the three-term combination, and the packer's
                            object-to-world product behind each corner (nothing where the matrix is the identity: then it is exact)
  emitter point, sphere     u (N_UNIT + N_AFFINE) sum_j |v_j m_j| + u N_AFFINE |t|: normalize, then the affine map
  emitter pdf, triangle     relative u (A_TRI + A_AREA S_c / h + (B_TRI_COS + B_TRI_POS thin S / dist) / |cos|): S the size of the numbers the hit point is
                            formed from (the larger of |origin| and the largest corner), dist the distance to the hit, thin the triangle's aspect
                            (transform_cases.TriangleSet.thin), cos between the ray and the emitter's plane
  emitter pdf, sphere       relative u A_SPH + dc / (1 - cos theta_max), dc the move of cos theta_max = sqrt(x), x = 1 - q, q = r^2 / d^2, with x
                            moved by (2 B_SPH_Q q + x) u either way -- to first order u cos theta_max (B_SPH_Q q / (1 - q) + B_SPH_ROOT): the
                            known size of the cancellation in 1 - sqrt(1 - q), continuous through the clamp at x = 0
  mixture                   relative u N_MIX on top of what pdf_bsdf and pdf_l bring
  direct_sample             the above, and the largest move of wi, pdf, distant and sampled when the position and the normal the device formed
                            in fp32 are moved by their budgets in the module's 16 sign patterns (_surface)

ASIDES.  A sample is an aside where a discrete decision lies within its budget of flipping: a rejection test of random_in_unit_sphere whose
fp64 len^2 is within REJECT_SLACK u of 1, a ray whose closest hit is anyone's (Tracer below: the budgets of transform_cases.Reference.trace's geometry), dot(wo, n) > 0 within the normal's budget,
the 1e-5 cut within the pdf's allowance, any discrete outcome that differs under the 16 patterns.  An aside is compared with the union of the
admissible answers, never skipped; the tests cap the share of asides per case at EDGE_CAP = 0.5 % from the reference alone.  One class is
outside the cap's count (not outside the check), by construction and not by result: a light sample on a flat emitter in whose plane the
position itself lies (direct_sample, `exempt`)."""
import numpy as np

import bsdf_reference as br
import transform_cases as tc
from rene_amd import abi

U = 2.0 ** -24
EDGE_CAP = 0.005  # gbuffer_reference.EDGE_CAP's figure
PI32 = br.PI      # the specification's fp32 literal

# ---- counted constants (u) ------------------------------------------------------------------------------------------------------------------------
N_COMBINE = 3.000001  # p0 b0 + p1 r + p2 s: gamma_3 of a three-term sum of products (product, sum, sum), fused or not (test_gpu_frame_stream.py)
N_XFORM = 4.0         # the packer's x m0 + y m3 + z m6 + t: three products, three sums, at most 4 u of the terms' magnitudes (gamma_4)
N_UNIT = 4.5          # v rsq(v.v): v.v 3 u relative (positive terms), halved by the root 1.5 u, rsq 2 u, the product 1 u (bsdf_reference (a))
N_AFFINE = 4.0        # aff_point: as N_XFORM
REJECT_SLACK = 4.0    # len^2 = a a + b b + c c of exact a, b, c: three roundings of numbers below 3, fused or not: 3 u relative, rounded up
# triangle pdf = qdiv(qdiv(d2, cosine * area), primitive_count):
#   A: ro - hit_pos 1 u per component -> 2 u on d2, the sum of squares 3 u, cosine * area 1 u, the packer's area 0.5 sqrt(c.c) with c a cross
#      product of fp32 edges (edges 1 u each, differences of products 2 u, c.c 3 u halved, the root 0.5 u: 8 u for the catalogue's triangles),
#      two qdiv 8 u                                                                                                                 => 22
#   A_AREA: where the packer formed the world corners (a matrix that is not the identity) each carries N_XFORM u S_c, an edge twice that, and
#      the area takes an edge's error over the height it spans: 2 edges x 2 corners x N_XFORM = 16 u S_c / h_min
#   B_COS: the absolute error of cosine = |normalize(rd) . n^| over the cosine: normalize 4.5 u, the dot product 3 u, the packer's unit normal
#      (a cross product through the fp32 inverse of a map of condition <= transform_cases.MAX_CONDITION, over its length: 16 u per component)  => 24
#   B_POS: the hit point p0 + u e1 + v e2 against the ray's fp64 point.  Both traversals place the origin against the plane with an error of
#      (3 + 3 + 1) u S over the cosine (item loop: n.o, n.p0 and their difference; Moeller-Trumbore: tv = o - p0, its dot product, the
#      cross product behind it), t itself 6 u / |cos| + 3 u relative, the in-plane coordinates 5 u S thin, the three-term reconstruction and the
#      rounded edges 6 u S: 24 u S / |cos| at most, and d2 takes a displacement twice over the distance                               => 48
A_TRI, A_AREA, B_TRI_COS, B_TRI_POS = 22.0, 16.0, 24.0, 48.0
# sphere pdf = rcp(2 pi (1 - sqrt(max(1 - qdiv(r r, |c - ro|^2), 0)))):
#   r = (|m0| + |m4| + |m8|) / 3: two sums 2 u, the quotient 5 u = 7 u; r r: 15 u; |c - ro|^2: differences of fp32 numbers 1 u each -> 2 u, the
#   sum of squares 3 u = 5 u; qdiv 4 u: q carries 24 u relative.  x = 1 - q: 24 u q + 1 u x absolute; c = sqrt(x): half of that over x, and
#   2 u; 1 - c: c (12 q / x + 0.5 + 2) u + 1 u (1 - c) absolute.  Then the product by 2 pi 1 u and rcp 2 u.
#   A = 1 + 1 + 2 = 4, B(q) = c (12 q / (1 - q) + 2.5)
A_SPH, B_SPH_Q, B_SPH_ROOT = 4.0, 12.0, 2.5
N_NORMALISE = 4.5     # one more normalize of the direction (rene_emitter_pdf_form's form 2): per component of a unit vector
N_MIX = 8.0           # 0.5 pdf + qdiv(0.5 pdf_l, n): the halves are exact, qdiv 4 u, (float) n exact, the sum 1 u; T / pdf below adds rcp 2 u + 1 u
CUT = float(np.float32(1e-5))


def _in(v):
    """(n, 3) float64 of an input: the fp32 numbers a device was handed, unless the caller hands float64 over (the reference's own position)."""
    v = np.asarray(v)
    return (v if v.dtype == np.float64 else v.astype(np.float32).astype(np.float64)).reshape(-1, 3)


# ---- the emit-object table ------------------------------------------------------------------------------------------------------------------------
class EmitObject:
    """One entry of the emit-object table: a sphere (its 4 x 4 object-to-world matrix, float64 of the ABI's fp32) or a triangle mesh (world
    corners in float64, per corner and component the size of the numbers the packer's fp32 product handled, and the (ntri, 3) indices)."""

    def __init__(self, scene, index, inst):
        self.instance, self.sphere = index, inst.shape == abi.SHAPE_SPHERE
        self.matrix = tc.instance_matrix(inst)
        if self.sphere:
            self.prim_count = 1
            return
        mesh = scene.meshes[inst.mesh_index]
        p = mesh.vertices[:, 0:3].astype(np.float64)
        lin, t = self.matrix[:3, :3], self.matrix[:3, 3]
        self.vertices = p @ lin.T + t
        identity = np.array_equal(lin, np.eye(3)) and not t.any()
        self.vscale = np.zeros_like(p) if identity else np.abs(p) @ np.abs(lin).T + np.abs(t)
        self.indices = np.asarray(mesh.indices).reshape(-1, 3).astype(np.int64)
        self.prim_count = len(self.indices)
        self.triangles = tc.TriangleSet(self.vertices[self.indices])
        c = self.vertices[self.indices]
        edges = np.stack([c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], c[:, 2] - c[:, 1]], 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.height = np.linalg.norm(self.triangles.n, axis=1) / np.linalg.norm(edges, axis=2).max(1)  # the smallest height
        self.moved = not identity
        un, off = self.triangles.unit_n, (self.triangles.unit_n * c[:, 0]).sum(1)
        self.flat = bool((np.abs(un - un[0]).max() < 1e-6) and (np.abs(off - off[0]).max() < 1e-6))  # every triangle in one plane


def emit_objects(scene):
    """The emit-object table in the packer's order: the instances with an area light that is not the null one, in instance order."""
    return [EmitObject(scene, i, inst) for i, inst in enumerate(scene.instances)
            if scene.area_lights[inst.area_light_index].type != abi.AREA_LIGHT_NULL]


# ---- the point on an emitter, surface_sample.rs:69-117 ----------------------------------------------------------------------------------------------
MAX_ROUNDS = 64  # of the rejection loop: a round accepts with probability pi / 6


def emitter_point(objects, obj, rng, idx=None):
    """The sampler of object obj[i] on stream i of `rng` (a bsdf_reference.Rng), for the samples `idx` (all of them by default).
    Returns a dict of (n, ...) arrays, rows outside idx zero: point, allow (per component, absolute), draws (u32 drawn here), aside, and the
    decisions: prim, r, s (after the fold), fold, rounds."""
    n = len(rng.state)
    obj = np.broadcast_to(np.asarray(obj, np.int64), (n,))
    idx = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    out = {"point": np.zeros((n, 3)), "allow": np.zeros((n, 3)), "draws": np.zeros(n, np.int64), "aside": np.zeros(n, bool),
           "prim": np.full(n, -1), "r": np.zeros(n), "s": np.zeros(n), "fold": np.zeros(n, bool), "rounds": np.zeros(n, np.int64)}
    before = rng.draws.copy()
    for k, e in enumerate(objects):
        w = idx[obj[idx] == k]
        if not len(w):
            continue
        if e.sphere:
            v = np.zeros((len(w), 3))
            todo = np.arange(len(w))
            for _ in range(MAX_ROUNDS):  # math.rs:8-20: -1 + 2 f is exact in fp32 (an integer of 25 bits at most over 2^24, even)
                c = np.stack([-1.0 + 2.0 * rng.f32(w[todo]) for _ in range(3)], 1)
                len2 = (c * c).sum(1)
                out["aside"][w[todo]] |= np.abs(len2 - 1.0) <= REJECT_SLACK * U
                out["rounds"][w[todo]] += 1
                ok = len2 < 1.0
                v[todo[ok]] = c[ok]
                todo = todo[~ok]
                if not len(todo):
                    break
            assert not len(todo), "a rejection loop of more than MAX_ROUNDS rounds"
            with np.errstate(invalid="ignore", divide="ignore"):
                unit = v / np.sqrt((v * v).sum(1))[:, None]  # (the centre itself, drawn with probability 2^-72, normalises to NaN on both sides)
            lin, t = e.matrix[:3, :3], e.matrix[:3, 3]
            out["point"][w] = unit @ lin.T + t
            terms = np.abs(unit) @ np.abs(lin).T
            out["allow"][w] = U * ((N_UNIT + N_AFFINE) * terms + N_AFFINE * np.abs(t))
            continue
        prim = (rng.u32(w) % np.uint64(e.prim_count)).astype(np.int64)  # Q6
        r, s = rng.f32(w), rng.f32(w)
        fold = (r.astype(np.float32) + s.astype(np.float32)) > np.float32(1.0)  # the fp32 sum decides, as the specification's does
        r, s = np.where(fold, 1.0 - r, r), np.where(fold, 1.0 - s, s)           # exact in fp32: multiples of 2^-24 in [0, 1]
        b0 = ((np.float32(1.0) - r.astype(np.float32)) - s.astype(np.float32)).astype(np.float64)
        corners, vs = e.vertices[e.indices[prim]], e.vscale[e.indices[prim]]
        b = np.stack([b0, r, s], 1)[:, :, None]
        out["point"][w] = (corners * b).sum(1)
        out["allow"][w] = U * (N_COMBINE * np.abs(corners * b).sum(1) + N_XFORM * (vs * np.abs(b)).sum(1))
        out["prim"][w], out["r"][w], out["s"][w], out["fold"][w] = prim, r, s, fold
    out["draws"] = rng.draws - before
    return out


def emit_sample(objects, seeds):
    """rene_emit_sample restated: fw = PCG32si::new(seed), obj = next_u32 % emit_object_len, the point, the stream's next u32."""
    rng = br.Rng(np.asarray(seeds, np.uint64))
    everyone = np.arange(len(rng.state))
    obj = (rng.u32(everyone) % np.uint64(len(objects))).astype(np.int64)
    out = emitter_point(objects, obj, rng)
    out["obj"] = obj
    out["next"] = rng.u32(everyone).astype(np.uint32)
    return out


def seed_for_draw(k, target):
    """A seed whose k-th next_u32 (k = 0: the first) is `target`, or None: bsdf_reference.seed_with's inversion, k steps further back
    (only every other state has a seed)."""
    s0 = br._unoutput(int(target))
    for _ in range(k):
        s0 = br._unstep(s0)
    r = (br._unstep(s0) - br._INC) & br.M32
    if r % 2:
        return None
    seed = (r // 2 * pow((br._MUL + 1) // 2, -1, 1 << 31)) % (1 << 31)
    s = br.pcg_new(seed)
    for _ in range(k):
        s = br._step(s)
    assert int(br._output(s)[0]) == int(target)
    return seed


# Seeds whose third and fourth draws -- r and s of a triangle object -- sum to 2^24 - 1, 2^24, 2^24 + 1 and 2^24 + 2 over 2^24, found by a
# search of the first 2^24 seeds (tests/test_light_reference.py checks the sums): (seed, r 2^24, s 2^24).  1 + 2^-24 is no fp32 number: the
# sum rounds to 1, `r + s > 1` is false, and b0 = 1 - r - s = -2^-24 -- the specification's own answer, a point 2^-24 outside the triangle.
SUM_SEEDS = {"below": (6119062, 5534545, 11242670), "one": (7786742, 4242043, 12535173), "above": (15723727, 16519728, 257489),
             "fold": (7764865, 13107260, 3669958)}


def seed_with_draw(k, targets):
    """The first of `targets` that has a seed: (seed, target)."""
    for t in targets:
        seed = seed_for_draw(k, t)
        if seed is not None:
            return seed, int(t)
    raise ValueError("no seed")


# ---- the closest hit, with asides that scale --------------------------------------------------------------------------------------------------------
# transform_cases.Reference.trace sets a ray aside by fixed thresholds made for the t, u, v of rene_trace (a plane within 1e-2 of the ray, a
# discriminant below 1e-3 of half_b^2): under them a third of the light samples on a sphere emitter (its limb) and every ray within 1e-2 rad of
# an emitter's plane would be asides.  The light side asks less of a hit -- which surface, and for a triangle a point whose error the pdf's own
# allowance carries over the cosine -- so the same brute-force geometry (transform_cases.ray_sphere, TriangleSet) is judged here by budgets:
#   sphere: disc = half_b^2 - a c in fp32 (the ball short form: oc 1 u per component, half_b 3 u more and squared: 9 u half_b^2; c = |oc|^2 -
#     r^2 5 u and a 3 u and the product: 9 u a |c| <= 9 u half_b^2 near a tangent; the general form places the origin in object space with
#     4 u S / D per component more, for S / D <= 2 another 32 u): |disc| / half_b^2 < DISC_SLACK = 64 u is a hit or a miss by rounding
#   triangle: the inside test's own numbers.  Moeller-Trumbore: u = (tv . pv) / det with tv = o - p0 (1 u S), pv = d x e2 (2 u), the dot
#     product 3 u: u (5 |tv| + S) |e2| / |det| <= 6 u S / (h |cos|), h the height onto the edge; item loop: the point o + t d lies 7 u S /
#     |cos| along the ray (beside B_TRI_POS) and its coordinates in the reciprocal basis take 5 u S / h more: EDGE_N = 12 u S / (h |cos|) at
#     most, in barycentric units: a hit that close to an edge is anyone's
#   t: a triangle's u ((7 S + 6 t) / |cos| + 3 t) (beside B_TRI_POS), a sphere's (|half_b| / a) u (16 / sqrt(disc / half_b^2) + 8) (the root takes
#     the discriminant's 18 u over twice its own size; the quotient and the sum): two surfaces within the sum of theirs tie, a root within its
#     own of tmin is an edge
DISC_SLACK = 64.0
EDGE_N = 12.0


class Tracer:
    """The closest hit of a Scene by brute force in float64 (which = 1: the emitter structure), as transform_cases.Reference, with `aside`."""

    def __init__(self, scene, which=0):
        self.spheres, self.meshes = [], []
        for i, inst in enumerate(scene.instances):
            if which and scene.area_lights[inst.area_light_index].type == abi.AREA_LIGHT_NULL:
                continue
            if inst.shape == abi.SHAPE_SPHERE:
                self.spheres.append((i, tc.instance_matrix(inst)))
            else:
                corners = tc.world_corners(scene, inst)
                ts = tc.TriangleSet(corners)
                e = np.stack([corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], corners[:, 2] - corners[:, 1]], 1)
                with np.errstate(invalid="ignore", divide="ignore"):
                    height = np.linalg.norm(ts.n, axis=1) / np.linalg.norm(e, axis=2).max(1)  # the smallest height
                self.meshes.append((i, ts, np.linalg.norm(corners, axis=2).max(1), height))

    def _candidates(self, o, d, tmin, tmax, chunk):
        """Yields (rows, instance, t, hit, event, dt, sure, u, v, prim, normal) per surface and chunk of rays, (len(rows), m) each.  t and hit:
        the float64 verdict.  event: the ray parameter at which the surface may be met within its budget (inf: not at all; -inf: an edge at
        tmin or tmax, always in the way).  sure: a hit by more than the budget.  dt: the budget of t."""
        n = len(o)
        everyone = np.arange(n)
        size_o = np.linalg.norm(o, axis=1)
        dlen = np.linalg.norm(d, axis=1)
        for i, m in self.spheres:
            t, normal, disc_n, roots = tc.ray_sphere(m, o, d, tmin, tmax)
            inv = np.linalg.inv(m[:3, :3])
            oc, od = (o - m[:3, 3]) @ inv.T, d @ inv.T
            a, half_b = (od * od).sum(1), (oc * od).sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                nearest = -half_b / a
                dt = np.nan_to_num(np.abs(nearest) * U * (16.0 / np.sqrt(np.maximum(np.abs(disc_n), DISC_SLACK * U)) + 8.0))
                tangent = (np.abs(disc_n) < DISC_SLACK * U) & (nearest > tmin - dt) & (nearest < tmax + dt)
                edge = (np.abs(roots - tmin) <= dt[:, None]).any(1) | (np.abs(roots - tmax) <= dt[:, None]).any(1)
            hit = ~np.isnan(t)
            event = np.where(edge, -np.inf, np.where(tangent, nearest, np.where(hit, t, np.inf)))
            col = lambda x: x[:, None]
            yield (everyone, i, col(np.where(hit, t, np.inf)), col(hit), col(event), col(dt), col(hit & ~tangent & ~edge),
                   np.zeros((n, 1)), np.zeros((n, 1)), np.zeros(1, np.int64), normal[:, None, :])
        for i, ts, size_c, height in self.meshes:
            for lo in range(0, n, chunk):
                rows = everyone[lo:lo + chunk]
                t, u, v, cos = ts.hits(o[rows], d[rows])
                dl = dlen[rows][:, None]
                with np.errstate(invalid="ignore", divide="ignore"):
                    S = np.maximum(size_o[rows][:, None], size_c[None, :])
                    ac = np.abs(cos)
                    slack = EDGE_N * U * S / (ac * height[None, :])
                    dt = np.nan_to_num(U * ((7.0 * S / dl + 6.0 * np.abs(t)) / ac + 3.0 * np.abs(t)), posinf=0.0)
                    low = np.minimum(np.minimum(u, v), 1.0 - u - v)
                    live = ts.live[None, :] & np.isfinite(t)
                    in_t = (t >= tmin) & (t <= tmax)
                    hit = live & (low >= 0.0) & in_t
                    near = live & (low >= -slack)
                    edge = near & ((np.abs(t - tmin) <= dt) | (np.abs(t - tmax) <= dt))
                    sure = hit & (low > slack) & ~edge
                    event = np.where(edge, -np.inf, np.where(near & in_t, t, np.inf))
                yield (rows, i, np.where(hit, t, np.inf), hit, event, dt, sure, u, v, np.arange(len(ts.p0)), ts.n[None, :, :])

    def trace(self, origins, directions, tmin=tc.TMIN, tmax=tc.TMAX, chunk=1024):
        o, d = _in(origins), _in(directions)
        n = len(o)
        out = {"t": np.full(n, np.inf), "u": np.zeros(n), "v": np.zeros(n), "instance": np.full(n, -1), "primitive": np.full(n, -1),
               "normal": np.zeros((n, 3)), "dt": np.zeros(n), "sure": np.zeros(n, bool)}
        for rows, i, t, hit, event, dt, sure, u, v, prim, normal in self._candidates(o, d, tmin, tmax, chunk):  # pass 1: the float64 verdict
            k = t.argmin(1)
            r = np.arange(len(rows))
            better = t[r, k] < out["t"][rows]
            w = rows[better]
            out["t"][w], out["dt"][w], out["instance"][w] = t[r, k][better], dt[r, k][better], i
            out["sure"][w] = sure[r, k][better]
            out["u"][w], out["v"][w], out["primitive"][w] = u[r, k][better], v[r, k][better], prim[k][better]
            out["normal"][w] = (normal[0, k] if normal.shape[0] == 1 else normal[r, k])[better]
        aside = np.zeros(n, bool)  # pass 2: anything unsure, or another surface, no farther than the budgets behind the hit
        rivals = {}  # ray -> [(instance, primitive, t)]: the other surfaces in the way, the alternative answers of an aside
        for rows, i, t, hit, event, dt, sure, u, v, prim, normal in self._candidates(o, d, tmin, tmax, chunk):
            reach = (out["t"][rows] + out["dt"][rows])[:, None] + dt
            is_hit = (out["instance"][rows][:, None] == i) & (prim[None, :] == out["primitive"][rows][:, None])
            in_way = (event <= reach) & (event < np.inf)
            aside[rows] |= (in_way & ~sure).any(1) | (in_way & ~is_hit).any(1)
            behind = np.zeros_like(in_way)  # a hit that may be a miss uncovers what lies behind it: the two nearest other surfaces of this lot
            shaky = np.nonzero(np.isfinite(out["t"][rows]) & ~out["sure"][rows])[0]
            if len(shaky):
                ev = np.where(is_hit[shaky] | in_way[shaky], np.inf, event[shaky])
                for _ in range(2):
                    k = ev.argmin(1)
                    some = np.isfinite(ev[np.arange(len(shaky)), k])
                    behind[shaky[some], k[some]] = True
                    ev[np.arange(len(shaky)), k] = np.inf
            for r, k in zip(*np.nonzero((in_way & ~is_hit) | behind)):
                rivals.setdefault(int(rows[r]), []).append((i, int(prim[k]), float(t[r, k]) if np.isfinite(t[r, k]) else max(float(event[r, k]), tmin)))
        found = np.isfinite(out["t"])
        out["aside"] = aside
        out["rivals"] = rivals
        out["grazing"] = aside  # (the name transform_cases.compare_hits reads)
        out["t"] = np.where(found, out["t"], -1.0)
        return out


# ---- the emitter pdf, lib.rs:959-1066 -----------------------------------------------------------------------------------------------------------------
def emitter_pdf(objects, hit, origins, directions, extra_normalise=False):
    """pdf_l of the rays (origins, directions: the fp32 numbers) whose closest hit in the emitter structure is `hit` (Tracer(scene, 1).trace of
    the same rays).  Returns (pdf, allow, aside): 0 for a miss; the triangle's d^2 / (|cos| area) / prim_count; the sphere's cone
    of quirk Q4, +inf for a zero quirk radius; allow absolute (inf where pdf is); aside where the hit is anyone's.  extra_normalise: the direction went through one more normalize on its way (form 2)."""
    o, d = _in(origins), _in(directions)
    n = len(o)
    pdf, rel, aside = np.zeros(n), np.zeros(n), np.asarray(hit["grazing"], bool).copy()
    dlen = np.linalg.norm(d, axis=1)
    for e in objects:
        w = np.nonzero((hit["t"] > 0) & (hit["instance"] == e.instance))[0]
        if not len(w):
            continue
        if e.sphere:
            m = e.matrix.astype(np.float32).astype(np.float64)
            radius = (abs(m[0, 0]) + abs(m[1, 1]) + abs(m[2, 2])) / 3.0
            d2 = ((m[:3, 3] - o[w]) ** 2).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = radius * radius / d2
                x = np.maximum(1.0 - q, 0.0)
                c = np.sqrt(x)
                pdf[w] = 1.0 / (2.0 * PI32 * (1.0 - c))
                # x moves by (24 q + x) u (beside A_SPH); the root of a number that small moves by more than its derivative says, and the
                # clamp at 0 is continuous: the root is taken at both ends of x's interval.  B_SPH_Q q / (1 - q) + B_SPH_ROOT is this to first order
                dx = (2.0 * B_SPH_Q * q + x) * U
                dc = np.maximum(np.sqrt(x + dx) - c, c - np.sqrt(np.maximum(x - dx, 0.0))) + (B_SPH_ROOT - 0.5) * U * c  # (the root's own 2 u)
                rel[w] = U * A_SPH + dc / (1.0 - c)
            continue
        ts, prim = e.triangles, hit["primitive"][w]
        normal = ts.unit_n[prim]
        area = 0.5 * np.linalg.norm(ts.n[prim], axis=1)
        dist = hit["t"][w] * dlen[w]
        cos = np.abs((d[w] * normal).sum(1)) / dlen[w]
        corners = e.vertices[e.indices[prim]]
        size = np.maximum(np.linalg.norm(o[w], axis=1), np.linalg.norm(corners, axis=2).max(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf[w] = dist * dist / (cos * area) / e.prim_count
            b_cos = B_TRI_COS + (N_NORMALISE if extra_normalise else 0.0)
            area_term = A_AREA * np.linalg.norm(corners, axis=2).max(1) / e.height[prim] if e.moved else 0.0
            rel[w] = U * (A_TRI + area_term + (b_cos + B_TRI_POS * ts.thin[prim] * size / dist) / cos)
    with np.errstate(invalid="ignore"):
        allow = np.where(np.isfinite(pdf), rel * pdf, np.inf)
    return pdf, allow, aside


def solid_angle_of_sphere(radius, distance):
    return 2.0 * np.pi * (1.0 - np.sqrt(1.0 - (radius / distance) ** 2))


# ---- the distant light's direction, light.rs:52-55 ---------------------------------------------------------------------------------------------------------
def distant_wi(position, direction):
    """wi = normalize((p + dir) - p): the sum and the difference in fp32 (the quirk is part of the specification: the difference keeps the bits
    of dir that survive at p's magnitude), the normalize in float64.  position: the fp32 position (n, 3); direction: the light's fp32 dir."""
    p = np.asarray(position, np.float32).reshape(-1, 3)
    target = p + np.asarray(direction, np.float32)
    v = (target - p).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=1)[:, None]


# ---- the mixture, lib.rs:316-320 -------------------------------------------------------------------------------------------------------------------------
def mixture(pdf_bsdf, pdf_l, n_objects, allow_bsdf=0.0, allow_l=0.0):
    """pdf = 0.5 pdf_bsdf + 0.5 pdf_l / emit_object_len (Q1, Q5) and the `< 1e-5` cut.  Returns (pdf, allow, ended, either): ended is the fp64
    decision, either where the pdf lies within its allowance of the cut -- both states are then admissible."""
    pdf_bsdf, pdf_l = np.asarray(pdf_bsdf, np.float64), np.asarray(pdf_l, np.float64)
    with np.errstate(invalid="ignore"):
        pdf = 0.5 * pdf_bsdf + 0.5 * pdf_l / n_objects
        allow = 0.5 * allow_bsdf + 0.5 * np.asarray(allow_l, np.float64) / n_objects + N_MIX * U * np.abs(pdf)
        allow = np.where(np.isfinite(pdf), allow, np.inf)
        ended = pdf < CUT
        either = np.abs(pdf - CUT) <= allow
    return pdf, allow, ended, either


def pdf_check(got, objects, hit, origins, directions, extra_normalise=False):
    """A device's (or the oracle's) pdf_l against emitter_pdf: (ok per ray, the largest |got - reference| / allowance over the rays that are no
    asides, the aside mask).  A miss wants exactly 0, an infinite pdf exactly +inf; an aside ray may also give 0 or the pdf of the other surface
    in its way (Tracer's `rivals`)."""
    got = np.asarray(got, np.float64)
    pdf, allow, aside = emitter_pdf(objects, hit, origins, directions, extra_normalise)
    with np.errstate(invalid="ignore"):
        err = np.where(np.isfinite(pdf), np.abs(got - pdf), np.where(got == pdf, 0.0, np.inf))
        ok = err <= allow
        o3, d3 = _in(origins), _in(directions)
        for i in np.nonzero(aside & ~ok)[0]:
            ok[i] = got[i] == 0.0
            for inst, prim, t in hit["rivals"].get(int(i), []):
                one = {"t": np.array([t]), "instance": np.array([inst]), "primitive": np.array([prim]), "grazing": np.zeros(1, bool)}
                pdf2, allow2, _ = emitter_pdf(objects, one, o3[i:i + 1], d3[i:i + 1], extra_normalise)
                ok[i] |= bool(np.abs(got[i] - pdf2[0]) <= allow2[0]) if np.isfinite(pdf2[0]) else bool(got[i] == pdf2[0])
        judged = ~aside & (pdf > 0) & np.isfinite(pdf)
        ratio = float((err[judged] / allow[judged]).max()) if judged.any() else 0.0
    return ok, ratio, aside


# ---- the cases of tests/test_light_reference.py (their aside shares) and tests/test_gpu_light_fp64.py ---------------------------------------------------
MAPS_MESH, MAPS_BALL = ("nonuniform", "sheared", "mirrored"), ("rotated", "nonuniform", "mirrored", "cyclic")
FILM = (48, 40)


def mixed_emitters():
    """Cornell with a sphere emitter under the `rotated` map of the catalogue beside its quad: one emit-object table that holds a triangle
    object (two triangles) and a sphere object, so both arms of the sampler and of the pdf are taken on one context."""
    from rene_amd import scenes
    s = scenes.cornell_box(*FILM)
    s.add_sphere(1.0, s.add_matte((0, 0, 0)), area_light=s.add_area_light_diffuse((4.0, 3.0, 2.0)), ctm=tc.ctm("rotated", (-0.45, 0.6, 0.3), size=0.15))
    return s


def _scene(case):
    from rene_amd import scenes
    kind, _, name = case.partition("/")
    if kind == "cornell":
        return scenes.cornell_box(*FILM)
    if kind == "cornell+sun":
        s = scenes.cornell_box(*FILM)
        s.add_light_distant((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))
        return s
    if kind == "many-emitters":
        from test_gpu_frame_stream import many_emitters
        return many_emitters()[0]
    if kind == "veach":
        return scenes.veach_mis(64, 36)
    if kind == "mixed":
        return mixed_emitters()
    if kind == "ball":
        return tc.emitter_room(name).with_resolution(*FILM)
    return tc.mesh_emitter_room(name, kind)  # "quad" or "mesh"


_scenes = {}


def scene(case):
    if case not in _scenes:
        _scenes[case] = _scene(case)
    return _scenes[case]


POINT_CASES = ("cornell", "many-emitters", "veach", "mixed") + tuple(f"ball/{m}" for m in MAPS_BALL) + \
    tuple(f"{k}/{m}" for k in ("quad", "mesh") for m in MAPS_MESH)
PDF_CASES = POINT_CASES
N_SEEDS = 4096


def _aimed(rng, centre, n, spread):  # test_gpu_probes.py's _aimed_rays
    org = np.stack([rng.uniform(-4, 12, n), rng.uniform(0.2, 6.0, n), rng.uniform(-8, 8, n)], 1).astype(np.float32)
    tgt = np.asarray(centre, np.float32) + rng.normal(size=(n, 3)).astype(np.float32) * spread
    d = tgt - org
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _random_unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def plane_rays(corners, rng, n, lo=2e-4, hi=1e-3):
    """Rays that meet triangles of `corners` (m, 3, 3) at lo .. hi radians from their plane (log-uniform), from 0.3 to 1.5 away, at points near
    their centroids (barycentrics 1/3 +- 0.1: at 2e-4 rad the hit point's budget is a tenth of a triangle of the room, and a ray whose hit
    may cross an edge is an aside)."""
    k = rng.integers(0, len(corners), n)
    b = 1.0 / 3.0 + rng.uniform(-0.1, 0.1, (n, 2))
    p0, e1, e2 = corners[k, 0], corners[k, 1] - corners[k, 0], corners[k, 2] - corners[k, 0]
    tgt = p0 + b[:, :1] * e1 + b[:, 1:] * e2
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    phi = rng.uniform(0, 2 * np.pi, n)[:, None]
    a = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    along = np.cos(phi) * a + np.sin(phi) * np.cross(nrm, a)
    eps = np.exp(rng.uniform(np.log(lo), np.log(hi), n))[:, None] * rng.choice([-1.0, 1.0], (n, 1))
    direction = np.cos(eps) * along + np.sin(eps) * nrm
    o = (tgt - direction * rng.uniform(0.3, 1.5, (n, 1))).astype(np.float32)
    d = tgt - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def far_rays(m, radius, rng, n, lo=2.0, hi=200.0):
    """Rays at the sphere under the 4 x 4 map m from lo .. hi times `radius` away (log-uniform), aimed inside 0.6 of it."""
    m = np.asarray(m, np.float64)
    o = (m[:3, 3] + _random_unit(rng, n) * radius * np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 1)))).astype(np.float32)
    tgt = (_random_unit(rng, n) * (0.6 * rng.random((n, 1)) ** (1 / 3))) @ m[:3, :3].T + m[:3, 3]
    d = tgt - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


_rays = {}


def pdf_rays(case):
    """The rays of a pdf case, float32 (origins, directions): the sets of test_gpu_probes.py and test_gpu_transforms.py with their grazing rays
    kept, per triangle emitter 256 rays within 1e-3 rad of its plane, per sphere emitter 512 origins at 2 to 200 radii."""
    if case in _rays:
        return _rays[case]
    s, rng = scene(case), np.random.default_rng(sum(map(ord, case)))
    kind, _, name = case.partition("/")
    sets = []
    if kind == "cornell":  # test_emitter_pdf_probe_triangles
        g, n = np.random.default_rng(6), 6000
        org = np.stack([g.uniform(-0.9, 0.9, n), g.uniform(0.05, 1.6, n), g.uniform(-0.9, 0.9, n)], 1).astype(np.float32)
        tgt = np.stack([g.uniform(-0.3, 0.3, n), np.full(n, 1.98), g.uniform(-0.3, 0.25, n)], 1).astype(np.float32)
        d = tgt - org
        sets.append((org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)))
    if kind == "veach":  # test_emitter_pdf_probe_spheres
        g = np.random.default_rng(5)
        sets += [_aimed(g, (0, 6.5, z), 4000, 0.3 * radius) for z, radius in ((-2.8, 1.0), (0.0, 0.5), (2.7, 0.05))]
    if kind == "ball":  # test_sphere_emitter_pdf
        m = tc.ctm(name, tc.EMITTER_AT, size=tc.EMITTER_SIZE)
        q = tc.quirk_radius(m)
        g = np.random.default_rng(8)
        sets.append(tc.emitter_rays(m, g, 4000, 2.2 if name == "cyclic" else min(2.2, q / 0.1)))
        sets.append(tc.emitter_rays(tc.ctm(name, (1.5, 0.4, 1.0), size=tc.EMITTER_SIZE), g, 400))
    if kind in ("quad", "mesh"):  # test_mesh_emitters
        emitter = next(i for i in s.instances if i.area_light_index)
        sets.append(tc.mesh_rays(tc.world_corners(s, emitter), np.random.default_rng(12), 4000))
    for e in emit_objects(s):
        if e.sphere:
            radius = tc.quirk_radius(e.matrix.astype(np.float32)) or float(np.cbrt(abs(np.linalg.det(e.matrix[:3, :3]))))
            sets.append(far_rays(e.matrix, radius, rng, 512))
            if kind in ("mixed", "many-emitters"):
                sets.append(far_rays(e.matrix, radius, rng, 1000, 1.5, 12.0))
        else:
            corners = e.vertices[e.indices]
            if kind != "mesh":  # (a flat emitter has a plane; the displaced sphere's triangles are 0.03 high, and at 1e-3 rad the hit point's
                sets.append(plane_rays(corners, rng, 256))  # budget spans several of them: the reference alone could not name the triangle)
            if kind in ("mixed", "many-emitters"):
                sets.append(tc.mesh_rays(corners, rng, 1000))
    _rays[case] = (np.concatenate([a for a, _ in sets]), np.concatenate([b for _, b in sets]))
    return _rays[case]


_pdf_refs = {}


def pdf_reference(case):
    """(objects, Tracer(scene, 1).trace of pdf_rays(case)), once per process."""
    if case not in _pdf_refs:
        o, d = pdf_rays(case)
        _pdf_refs[case] = (emit_objects(scene(case)), Tracer(scene(case), 1).trace(o, d))
    return _pdf_refs[case]


# ---- the direct-light pass on Lambert surfaces: steps 3 to 7 of the header's specification ----------------------------------------------------------------
MISS, LIGHT, BSDF, PLAIN, ENDED_PDF, ENDED_ZERO = range(6)          # rene_direct_sample.state
SECOND_NONE, SECOND_MISS, SECOND_SURFACE, SECOND_EMITTER = range(4)  # rene_direct_sample.second
N_SHADING = 12.0  # the unit normal: three products and two sums of the corners' normals 3 u, two normalize 9 u
N_DIRECTION = 6.0  # wi = normalize(point - position): the difference 1 u, normalize 4.5 u, rounded up; per component of a unit vector
N_THROUGHPUT = 8.0  # T = f |n.wi| / pdf: f = R / pi 2 u (bsdf_reference.N), the dot product 3 u (absolute, taken over the cosine), rcp 2 u, the product 1 u
_PATTERNS = np.random.default_rng(20251).choice([-1.0, 1.0], (br.N_PATTERNS, 6))  # position and normal, the module's 16 sign patterns


class DirectScene:
    """What direct_sample reads of a Scene: camera origin, lights, emit objects, tracers, per instance the Lambert reflectance (None: not a
    single Lambert lobe), the emission, world corners and world shading normals."""

    def __init__(self, scene):
        self.scene = scene
        self.origin = np.asarray(scene.camera_to_world, np.float32)[:3, 3].astype(np.float64)
        self.objects = emit_objects(scene)
        self.main, self.emit = Tracer(scene, 0), Tracer(scene, 1)
        self.lights = [(np.asarray(l.v0[:3], np.float32), np.asarray(l.v1[:3], np.float64)) for l in scene.lights]
        self.R, self.L, self.corners, self.normals, self.matrix = [], [], [], [], []
        for inst in scene.instances:
            mat = scene.materials[inst.material_index]
            lambert = mat.type == abi.MATERIAL_MATTE and scene.textures[mat.u0[0]].type == abi.TEXTURE_SOLID
            self.R.append(np.asarray(scene.textures[mat.u0[0]].v0[:3], np.float64) if lambert else None)
            al = scene.area_lights[inst.area_light_index]
            self.L.append(np.asarray(al.v0[:3], np.float64) if al.type != abi.AREA_LIGHT_NULL else None)
            m = tc.instance_matrix(inst)
            self.matrix.append(m)
            if inst.shape == abi.SHAPE_SPHERE:
                self.corners.append(None)
                self.normals.append(None)
                continue
            mesh = scene.meshes[inst.mesh_index]
            idx = np.asarray(mesh.indices).reshape(-1, 3).astype(np.int64)
            c = tc.world_corners(scene, inst)
            inv_t = np.linalg.inv(m[:3, :3]).T
            vn = mesh.vertices[:, 3:6].astype(np.float64)[idx]             # (m, 3, 3) object-space vertex normals
            flat = ~vn.any(axis=(1, 2))                                    # all three zero: the geometric normal (scene_pack.cpp)
            po = mesh.vertices[:, 0:3].astype(np.float64)[idx]
            ng = np.cross(po[:, 1] - po[:, 0], po[:, 2] - po[:, 0])
            vn[flat] = ng[flat][:, None, :]
            self.corners.append(c)
            self.normals.append(vn @ inv_t.T)                               # M^-T n per corner


_direct_scenes = {}


def direct_scene(scene):
    if id(scene) not in _direct_scenes:
        _direct_scenes[id(scene)] = DirectScene(scene)
    return _direct_scenes[id(scene)]


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _surface(ds, inst, prim, o, d, t_hint):
    """Position, unit shading normal and their per-component budgets for rays (o, d) that met primitive `prim` of instance `inst`: the float64
    intersection of the ray with THAT primitive.  Budgets: the position as three moves (n, 3, 3).  A triangle's point p0 + u e1 + v e2 lies in
    the plane to its own three roundings and the packer's corners (N_COMBINE + N_XFORM) u S, and anywhere in the plane within the traversal's
    error of the hit point, (B_TRI_POS / 2) u S / |cos| (the count beside B_TRI_POS): two in-plane moves and one along the normal.  A
    sphere's point ro + t rd moves along the ray by the root's budget (Tracer) and across it by 2 u S.  The normal: N_SHADING u, and what
    the position's moves do to an interpolated or a sphere's normal."""
    n = len(o)
    pos, nrm, bpos, bnrm = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 1))
    for i in np.unique(inst):
        w = np.nonzero(inst == i)[0]
        m = ds.matrix[i]
        if ds.corners[i] is None:
            inv = np.linalg.inv(m[:3, :3])
            _, _, _, roots = tc.ray_sphere(m, o[w], d[w], -np.inf, np.inf)
            t = np.where(np.abs(roots[:, 0] - t_hint[w]) <= np.abs(roots[:, 1] - t_hint[w]), roots[:, 0], roots[:, 1])
            pos[w] = o[w] + t[:, None] * d[w]
            p_obj = (pos[w] - m[:3, 3]) @ inv.T
            raw = p_obj @ inv
            nrm[w] = _unit(raw)
            size = np.maximum(np.linalg.norm(o[w], axis=1), np.linalg.norm(pos[w], axis=1))
            cos = np.abs((_unit(d[w]) * nrm[w]).sum(1))
            oc, od = (o[w] - m[:3, 3]) @ inv.T, d[w] @ inv.T
            a, half_b = (od * od).sum(1), (oc * od).sum(1)
            disc_n = np.abs((half_b * half_b - a * ((oc * oc).sum(1) - 1.0)) / (half_b * half_b))
            along = np.abs(half_b / a) * U * (16.0 / np.sqrt(np.maximum(disc_n, DISC_SLACK * U)) + 8.0) * np.linalg.norm(d[w], axis=1) + 2.0 * U * size
            dh = _unit(d[w])
            t1 = _unit(np.cross(dh, np.where(np.abs(dh[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])))
            bpos[w, 0], bpos[w, 1], bpos[w, 2] = dh * along[:, None], t1 * (2.0 * U * size)[:, None], np.cross(dh, t1) * (2.0 * U * size)[:, None]
            bnrm[w, 0] = N_SHADING * U + along / np.maximum(cos, 1e-30) * np.linalg.norm(inv, 2) ** 2 / np.linalg.norm(raw, axis=1)
            continue
        c, vn = ds.corners[i][prim[w]], ds.normals[i][prim[w]]
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        ng = np.cross(e1, e2)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = ((c[:, 0] - o[w]) * ng).sum(1) / (d[w] * ng).sum(1)
            pos[w] = o[w] + t[:, None] * d[w]
            n2 = (ng * ng).sum(1)[:, None]
            u = ((pos[w] - c[:, 0]) * np.cross(e2, ng) / n2).sum(1)
            v = ((pos[w] - c[:, 0]) * np.cross(ng, e1) / n2).sum(1)
            raw = vn[:, 0] * (1.0 - u - v)[:, None] + vn[:, 1] * u[:, None] + vn[:, 2] * v[:, None]
            nrm[w] = _unit(raw)
            size = np.maximum(np.linalg.norm(o[w], axis=1), np.linalg.norm(c, axis=2).max(1))
            cos = np.abs((_unit(d[w]) * _unit(ng)).sum(1))
            in_plane = 0.5 * B_TRI_POS * U * size / np.maximum(cos, 1e-30)
            gn = _unit(ng)
            t1 = _unit(e1)
            bpos[w, 0], bpos[w, 1] = t1 * in_plane[:, None], np.cross(gn, t1) * in_plane[:, None]
            bpos[w, 2] = gn * ((N_COMBINE + N_XFORM) * U * size)[:, None]
            height = np.sqrt(n2[:, 0]) / np.linalg.norm(np.stack([e1, e2, e2 - e1], 1), axis=2).max(1)
            vary = np.linalg.norm(np.stack([_unit(vn[:, 1]) - _unit(vn[:, 0]), _unit(vn[:, 2]) - _unit(vn[:, 0])], 1), axis=2).max(1)
            bnrm[w, 0] = N_SHADING * U + in_plane / height * vary
    return pos, nrm, bpos, bnrm


def _lambert(R, n, wo, wi):
    """Bsdf::f(wo, wi) and the integrator's Bsdf::pdf(wi, normal) (Q1) of one Lambert lobe about the unit normal n (reflection.rs:286-342,
    bxdf.rs:87-113): f = R / pi where wo and wi lie on one side of the surface and wo is not in it; pdf = |n.n| / pi = 1 / pi where wi lies
    on the normal's side, else 0 -- the `wo` of that call is wi and its `wi` the normal itself."""
    cwi, cwo = (wi * n).sum(1), (wo * n).sum(1)
    f = np.where(((cwi * cwo > 0) & (cwo != 0))[:, None], R * br.INV_PI, 0.0)
    return f, np.where(cwi > 0, br.INV_PI, 0.0), cwi, cwo


def _direct_once(ds, seeds, wi_dev, inst, pos, nrm, wo, light, pt):
    """Steps 3 to 7 at one (position, normal): a dict of per-sample arrays."""
    n = len(pos)
    R = np.stack([ds.R[i] for i in inst])
    out = {}
    Lp = np.stack([ds.L[i] if ds.L[i] is not None else np.zeros(3) for i in inst])
    out["seen"] = np.where(((wo * nrm).sum(1) > 0)[:, None], Lp, 0.0)
    out["distant"], out["distant_allow"], q_aside = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, bool)
    for direction, L in ds.lights:  # step 4
        wi_d = distant_wi(pos.astype(np.float32), direction)
        sh = ds.main.trace(pos, wi_d, tc.TMIN, 1e5)
        q_aside |= sh["aside"]
        f, _, cwi, _ = _lambert(R, nrm, wo, wi_d)
        term = np.where((sh["t"] < 0)[:, None], f * np.abs(cwi)[:, None] * L, 0.0)
        out["distant"] += term
        # wi_d: the fp32 sum and difference at a position a few ulps off differ by an ulp of |p| + 1 each: 4 u (|p| + 1), and normalize 4.5 u
        dw = U * (4.0 * (np.abs(pos).max(1) + 1.0) + N_UNIT + N_SHADING)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["distant_allow"] += term * ((N_THROUGHPUT + 2.0) * U + np.where(cwi != 0, np.sqrt(3.0) * dw / np.abs(cwi), 0.0))[:, None]
    # step 5
    with np.errstate(invalid="ignore", divide="ignore"):
        to_light = pt["point"] - pos
        dist = np.linalg.norm(to_light, axis=1)
        wi = np.where(light[:, None], to_light / dist[:, None], wi_dev)
        out["wi_allow"] = np.where(light, np.linalg.norm(pt["allow"], axis=1) / dist + np.sqrt(3.0) * N_DIRECTION * U, 0.0)
    f, pdf_q1, cwi, cwo = _lambert(R, nrm, wo, wi)
    # the BSDF branch's own sample (bxdf.rs:91-105): f = R / pi, pdf = |wi.z| / pi of the local wi, which the world wi and the normal give back
    # to BUDGET_WORLD + N_SHADING u
    f = np.where(light[:, None], f, R * br.INV_PI)
    pdf_b = np.where(light, pdf_q1, np.abs(cwi) * br.INV_PI)
    allow_b = np.where(light, N_SHADING * U * pdf_q1, (br.BUDGET_WORLD + N_SHADING + br.N["lambert.pdf"]) * U * br.INV_PI)
    eh = ds.emit.trace(pos, wi)
    pdf_l, allow_l, aside_l = emitter_pdf(ds.objects, eh, pos, wi)
    q_aside |= aside_l
    pdf, allow, ended, either = mixture(pdf_b, pdf_l, len(ds.objects), allow_b, allow_l)
    with np.errstate(invalid="ignore", divide="ignore"):
        T = f * (np.abs(cwi) / pdf)[:, None]
        T_rel = N_THROUGHPUT * U + np.where(cwi != 0, np.sqrt(3.0) * (N_SHADING * U + out["wi_allow"]) / np.abs(cwi), 0.0) + allow / pdf
    zero = ~T.any(1)
    state = np.where(ended, ENDED_PDF, np.where(zero, ENDED_ZERO, np.where(light, LIGHT, BSDF)))
    alive = ~ended & ~zero
    second, sampled = np.full(n, SECOND_NONE), np.zeros((n, 3))
    a = np.nonzero(alive)[0]
    if len(a):  # step 7
        h2 = ds.main.trace(pos[a], wi[a])
        q_aside[a] |= h2["aside"]
        second[a] = np.where(h2["t"] < 0, SECOND_MISS, SECOND_SURFACE)
        hit = np.nonzero(h2["t"] > 0)[0]
        emits = np.array([ds.L[i] is not None for i in h2["instance"][hit]], bool)
        k = hit[emits]
        if len(k):
            _, n2, _, _ = _surface(ds, h2["instance"][k], h2["primitive"][k], pos[a][k], wi[a][k], h2["t"][k])
            facing = (-(wi[a][k]) * n2).sum(1) > 0
            second[a[k]] = SECOND_EMITTER
            Le = np.stack([ds.L[i] for i in h2["instance"][k]])
            sampled[a[k]] = np.where(facing[:, None], T[a[k]] * Le, 0.0)
    out.update(state=state, second=second, wi=wi, pdf=pdf, pdf_allow=allow, either=either, sampled=sampled,
               sampled_allow=np.abs(sampled) * np.nan_to_num(T_rel, posinf=0.0)[:, None], query_aside=q_aside, light=light)
    return out


def direct_sample(scene, frame_seeds, primary_hits, device_wi):
    """Steps 3 to 7 of the direct-light pass for the samples whose primary hit is a single Lambert lobe.  frame_seeds (n,): the frame seed of
    every sample; primary_hits (n,) records of abi.PRIMARY_HIT_DTYPE (the device's own: d, t, instance, primitive); device_wi (n, 3): the
    mixture ray's direction as the device (or the BSDF reference) sampled it, read for the BSDF-state rows only.  Returns a dict: rows (the
    samples judged), and per row state, second, wi, pdf, seen, distant, sampled, their allowances (wi_allow: an angle), `aside`, and
    `exempt` (asides by construction, outside the cap's count), and `patterns`: the 16 perturbed evaluations an aside is compared with."""
    ds = direct_scene(scene)
    ph = np.asarray(primary_hits).reshape(-1)
    lam = np.array([ds.R[i] is not None for i in range(len(scene.instances))], bool)
    rows = np.nonzero((ph["t"] >= 0) & lam[np.minimum(ph["instance"], len(lam) - 1)])[0]
    inst, prim = ph["instance"][rows].astype(np.int64), ph["primitive"][rows].astype(np.int64)
    d = ph["d"][rows].astype(np.float64)
    o = np.broadcast_to(ds.origin, d.shape)
    pos, nrm, bpos, bnrm = _surface(ds, inst, prim, o, d, ph["t"][rows].astype(np.float64))
    wo = -_unit(d)
    seeds = np.asarray(frame_seeds, np.uint64).reshape(-1)[rows]
    fw = br.Rng(seeds)                                   # Q3: the frame-wide stream
    everyone = np.arange(len(rows))
    light = fw.f32(everyone) > 0.5
    li = everyone[light]
    obj = np.zeros(len(rows), np.int64)
    obj[li] = (fw.u32(li) % np.uint64(len(ds.objects))).astype(np.int64)
    pt = emitter_point(ds.objects, obj, fw, li)
    wi_dev = _in(device_wi)[rows]
    base = _direct_once(ds, seeds, wi_dev, inst, pos, nrm, wo, light, pt)
    patterns = [_direct_once(ds, seeds, wi_dev, inst, pos + (bpos * s[:3, None]).sum(1), _unit(nrm + bnrm * s[3:]), wo, light, pt) for s in _PATTERNS]
    flipped = np.zeros(len(rows), bool)
    spread = {k: np.zeros_like(base[k]) for k in ("pdf", "sampled", "distant")}
    turn = np.zeros(len(rows))
    for p in patterns:
        flipped |= (p["state"] != base["state"]) | (p["second"] != base["second"]) | (p["seen"] != base["seen"]).any(1)
        flipped |= (p["sampled"] != 0).any(1) != (base["sampled"] != 0).any(1)
        flipped |= (p["distant"] != 0).any(1) != (base["distant"] != 0).any(1)
        for k in spread:
            spread[k] = np.fmax(spread[k], br._spread(base[k], p[k]))
        with np.errstate(invalid="ignore"):
            turn = np.fmax(turn, np.nan_to_num(np.linalg.norm(p["wi"] - base["wi"], axis=1)))
    for k in spread:  # the allowance: the quantity's own roundings, and the largest move under the 16 patterns
        base[k + "_allow"] = base[k + "_allow"] + spread[k]
    base["wi_allow"] = base["wi_allow"] + turn
    base["aside"] = flipped | base["query_aside"] | base["either"] | pt["aside"]
    # Exempt from the cap's count, not from the check: a light sample drawn on a flat emitter in whose plane the position itself lies (the
    # emitter the primary ray hit, or one beside it on the same wall).  wi then lies in that plane by construction -- its cosine with the
    # emitter's normal is a rounding of zero on either side and the emitter query runs inside the plane -- so a case that shows such an
    # emitter to the camera holds these samples in proportion to its share of the film.
    exempt = np.zeros(len(rows), bool)
    for k, e in enumerate(ds.objects):
        if not e.sphere and e.flat:
            un, c0 = e.triangles.unit_n[0], e.vertices[e.indices[0, 0]]
            in_plane = np.abs(((pos - c0) * un).sum(1)) <= 2.0 * (N_COMBINE + N_XFORM) * U * np.maximum(np.linalg.norm(pos, axis=1), np.linalg.norm(c0))
            exempt |= light & (obj == k) & in_plane
    base["exempt"] = exempt
    base["rows"], base["patterns"], base["position"], base["normal"] = rows, patterns, pos, nrm
    return base


def direct_check(samples, ref):
    """The device's rene_direct_sample records (flattened like the primary hits direct_sample was given) against direct_sample's result:
    (ok per judged row, {quantity: the largest |device - reference| / allowance over the rows that are no asides}).  A row that is no aside
    wants state and second equal, seen equal bit for bit (an emission or 0), wi within wi_allow (an angle), pdf, distant and sampled within
    their allowances.  An aside row passes if it does so against the base or any of the 16 perturbed evaluations; one whose aside is a
    query's (a hit that is anyone's) is held to wi and seen."""
    s = np.asarray(samples).reshape(-1)[ref["rows"]]

    def against(r, allow):
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios = {"wi": np.where(ref["light"], np.linalg.norm(s["wi"].astype(np.float64) - r["wi"], axis=1) / allow["wi_allow"], 0.0),
                      "pdf": np.abs(s["pdf"].astype(np.float64) - r["pdf"]) / allow["pdf_allow"]}
            for k in ("sampled", "distant"):
                err = np.abs(s[k].astype(np.float64) - r[k])
                ratios[k] = np.where(err == 0, 0.0, err / allow[k + "_allow"]).max(1)
            ratios["pdf"] = np.where(s["pdf"].astype(np.float64) == r["pdf"], 0.0, ratios["pdf"])
        ok = (s["state"] == r["state"]) & (s["second"] == r["second"]) & (s["seen"].astype(np.float64) == r["seen"]).all(1)
        for k in ratios:
            ok &= np.nan_to_num(ratios[k], nan=np.inf) <= 1.0
        return ok, ratios

    ok, ratios = against(ref, ref)
    union = ok.copy()
    for p in ref["patterns"]:
        union |= against(p, ref)[0]
    loose = (np.nan_to_num(ratios["wi"], nan=np.inf) <= 1.0) & (s["seen"].astype(np.float64) == ref["seen"]).all(1)
    passed = np.where(ref["aside"], union | (ref["query_aside"] & loose), ok)
    judged = ~ref["aside"]
    worst = {k: float(np.nan_to_num(v[judged], nan=np.inf).max()) if judged.any() else 0.0 for k, v in ratios.items()}
    return passed, worst


def reference_wi(scene, frame_seeds, primary_hits, W, H):
    """The mixture ray's direction of every sample as the BSDF reference samples it (bsdf_reference.sample on the pixel's stream
    PCG32si::new((py W + px) ^ seed) behind its two jitter draws), (n, 3) float64, zero where the primary hit is no Lambert surface: what
    stands in for the device's wi where there is no device.  primary_hits: (frames, H, W) flattened, rows top first."""
    ds = direct_scene(scene)
    ph = np.asarray(primary_hits).reshape(-1)
    n = len(ph)
    pix = np.arange(n) % (W * H)
    py, px = H - 1 - pix // W, pix % W
    seeds = ((py * W + px).astype(np.uint64) ^ np.asarray(frame_seeds, np.uint64).reshape(-1)) & np.uint64(0xFFFFFFFF)
    lam = np.array([r is not None for r in ds.R], bool)
    rows = np.nonzero((ph["t"] >= 0) & lam[np.minimum(ph["instance"], len(lam) - 1)])[0]
    inst = ph["instance"][rows].astype(np.int64)
    d = ph["d"][rows].astype(np.float64)
    _, nrm, _, _ = _surface(ds, inst, ph["primitive"][rows].astype(np.int64), np.broadcast_to(ds.origin, d.shape), d, ph["t"][rows].astype(np.float64))
    out = np.zeros((n, 3))
    mats = np.array([scene.instances[i].material_index for i in inst])
    for m in np.unique(mats):
        k = np.nonzero(mats == m)[0]
        out[rows[k]] = br.sample(scene, int(m), nrm[k], np.zeros((len(k), 2), np.float32), -_unit(d[k]), seeds[rows[k]], skip=2).wi
    return out


# the direct-sample cases: name -> frames (the coin of depth 0 is the frame's, quirk Q3: enough frames for both of its sides)
DIRECT_CASES = {"cornell": 8, "cornell+sun": 4, "many-emitters": 4, "ball/uniform": 4}


def direct_inputs(case, n_frames, seed=abi.DEFAULT_SEED):
    """The frame seed of every sample of frames 0 .. n_frames - 1, flattened (frame, row, column)."""
    from rene_amd import api
    s = scene(case)
    return np.repeat(api.frame_seeds(seed, 0, n_frames), s.film.xresolution * s.film.yresolution)


def emitter_cosine(scene_, ref):
    """|cos| between wi and the emitter's geometric normal where the emitter query of a judged row hits (NaN elsewhere): how the tests count
    the samples that graze the light."""
    ds = direct_scene(scene_)
    eh = ds.emit.trace(ref["position"], ref["wi"])
    with np.errstate(invalid="ignore"):
        return np.where(eh["t"] > 0, np.abs((_unit(eh["normal"]) * ref["wi"]).sum(1)), np.nan)

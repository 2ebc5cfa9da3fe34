"""Test helper (not a conftest): the geometry pass (rene_gbuffer, include/rene_hip.h) restated in numpy.

`aggregate` turns per-sample records -- the device's own rene_primary_hits, or the oracle's -- into pixel records by the header's rules: fp32 running
sums in frame order, the position o + t d as a rounded multiply and a rounded add, fminf from +inf, the four id slots by the streaming rule, the
final ranking.  `reference_samples` makes the samples from the oracle alone: the seed schedule (PCG32si outputs of the master seed), pcg_f32 of
(y W + x) ^ seed, u = (x + r0) / (W - 1), v = (y + r1) / (H - 1), Oracle.camera_ray, Oracle.trace -- (x, y) the launch id, y counted from the
image's bottom row: record row = H - 1 - y.  It also marks the *edge samples*: those whose four oracle rays through (u +- DELTA, v +- DELTA) do
not all report what the centre ray reports (hit or miss, instance, primitive)."""
import numpy as np

from rene_amd import abi

DELTA = 4e-6        # ~ 30 fp32 ulps of a film coordinate near 1, 3e-4 of a pixel at 77 columns
EDGE_CAP = 0.005    # edge samples are at most this share of a scene's samples
ID_NAMES = ("instance", "material", "primitive")
NONE = np.uint32(0xFFFFFFFF)


def _bits(a):
    """The bit patterns of fp32 or uint32 values: what the per-pixel passes' tests (geometry, occlusion, direct light) compare."""
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_records_equal(got, want, what):
    """Two arrays of one pass's records, field by field and then byte for byte."""
    for k in got.dtype.names:
        bad = _bits(got[k]) != _bits(want[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got.tobytes() == want.tobytes(), what


def instance_materials(scene) -> np.ndarray:
    packed = scene.to_desc() if hasattr(scene, "to_desc") else scene
    d = packed.desc if hasattr(packed, "desc") else packed
    return np.array([d.instances[i].material_index for i in range(d.n_instances)], np.uint32)


def camera_origin(scene) -> np.ndarray:
    """The translation column of camera_to_world (column-major 4 x 4)."""
    packed = scene.to_desc() if hasattr(scene, "to_desc") else scene
    d = packed.desc if hasattr(packed, "desc") else packed
    return np.array(list(d.uniform.camera_to_world)[12:15], np.float32)


def sample_ids(samples, ids: str, materials=None) -> np.ndarray:
    if ids == "instance":
        return samples["instance"].astype(np.uint32)
    if ids == "primitive":
        return samples["primitive"].astype(np.uint32)
    if ids == "material":
        return np.asarray(materials, np.uint32)[samples["instance"]]
    raise ValueError(ids)


def aggregate(samples, origin, ids="instance", materials=None, owned=None) -> np.ndarray:
    """samples: (n, H, W) records with d (3), t (-1: a miss), instance, primitive, in frame order; origin: the rays' origin (3,) or per-sample
    (n, H, W, 3).  owned: (H, W) bool, the pixels of the tiles the context owns (default all); the others get the all-zero record."""
    samples = np.asarray(samples)
    n, H, W = samples.shape
    out = np.zeros((H, W), abi.GBUFFER_DTYPE)
    o = np.broadcast_to(np.asarray(origin, np.float32), (n, H, W, 3))
    depth_sum = np.zeros((H, W), np.float32)
    depth_min = np.full((H, W), np.inf, np.float32)
    pos = np.zeros((H, W, 3), np.float32)
    hits = np.zeros((H, W), np.uint32)
    other = np.zeros((H, W), np.uint32)
    slot_id = np.full((H, W, 4), NONE, np.uint32)
    count = np.zeros((H, W, 4), np.uint32)
    sid_all = sample_ids(samples, ids, materials)
    for f in range(n):
        t = samples["t"][f].astype(np.float32)
        hit = t >= 0
        d = samples["d"][f].astype(np.float32)
        p = o[f] + t[:, :, None] * d  # two fp32 ufuncs: a rounded multiply, then a rounded add
        hits += hit
        depth_sum = np.where(hit, depth_sum + t, depth_sum)
        depth_min = np.where(hit, np.fmin(depth_min, t), depth_min)
        pos = np.where(hit[:, :, None], pos + p, pos)
        sid = sid_all[f]
        todo = hit.copy()
        for k in range(4):  # the id is already in a slot
            m = todo & (count[:, :, k] > 0) & (slot_id[:, :, k] == sid)
            count[:, :, k] += m
            todo &= ~m
        for k in range(4):  # else the lowest free slot
            m = todo & (count[:, :, k] == 0)
            slot_id[:, :, k] = np.where(m, sid, slot_id[:, :, k])
            count[:, :, k] += m
            todo &= ~m
        other += todo       # else `other`
    # count descending, ties by id ascending (an unused slot -- count 0, id ~0 -- last)
    order = np.lexsort((slot_id, -count.astype(np.int64)), axis=-1)
    slot_id, count = np.take_along_axis(slot_id, order, -1), np.take_along_axis(count, order, -1)
    out["depth_sum"], out["depth_min"], out["hits"], out["n"] = depth_sum, depth_min, hits, n
    out["position_sum"], out["other"], out["id"], out["count"] = pos, other, slot_id, count
    if owned is not None:
        out[~np.asarray(owned, bool)] = np.zeros((), abi.GBUFFER_DTYPE)
    return out


def owned_mask(W, H, shard_rank=0, shard_count=1) -> np.ndarray:
    """The pixels of the 32 x 32 tiles with index % shard_count == shard_rank (rows top first)."""
    tiles_x = (W + 31) // 32
    y, x = np.mgrid[0:H, 0:W]
    return ((y // 32) * tiles_x + x // 32) % shard_count == shard_rank


def frame_seeds(oracle_mod, master_seed, first_frame, n_frames) -> np.ndarray:
    """The seed of global frame g is the g-th next_u32 of PCG32si::new(master)."""
    return oracle_mod.pcg_u32(master_seed, first_frame + n_frames)[first_frame:]


def film_coordinates(oracle_mod, W, H, seed):
    """(u, v), (H, W) each, rows top first, of the frame with this seed -- fp32 as the reference's ray generation computes them."""
    u = np.empty((H, W), np.float32)
    v = np.empty((H, W), np.float32)
    for row in range(H):
        y = H - 1 - row
        for x in range(W):
            r = oracle_mod.pcg_f32(((y * W + x) ^ int(seed)) & 0xFFFFFFFF, 2)
            u[row, x] = (np.float32(x) + r[0]) / np.float32(W - 1)
            v[row, x] = (np.float32(y) + r[1]) / np.float32(H - 1)
    return u, v


def _rays(oracle, u, v):
    o = np.empty(u.shape + (3,), np.float32)
    d = np.empty(u.shape + (3,), np.float32)
    for i in np.ndindex(u.shape):
        o[i], d[i] = oracle.camera_ray(float(u[i]), float(v[i]))
    return o, d


def _same(a, b):
    miss_a, miss_b = a["t"] < 0, b["t"] < 0
    return (miss_a == miss_b) & (miss_a | ((a["instance"] == b["instance"]) & (a["primitive"] == b["primitive"])))


def reference_samples(oracle_mod, oracle, W, H, first_frame, n_frames, master_seed=abi.DEFAULT_SEED, edges=True):
    """The oracle's samples of frames first_frame .. + n_frames - 1: a dict with `samples` (n, H, W) of abi.PRIMARY_HIT_DTYPE, `origin`
    (n, H, W, 3), `uv` (n, H, W, 2) and `edge` (n, H, W) bool (all False without `edges`)."""
    samples = np.zeros((n_frames, H, W), abi.PRIMARY_HIT_DTYPE)
    origin = np.zeros((n_frames, H, W, 3), np.float32)
    uv = np.zeros((n_frames, H, W, 2), np.float32)
    edge = np.zeros((n_frames, H, W), bool)
    for f, seed in enumerate(frame_seeds(oracle_mod, master_seed, first_frame, n_frames)):
        u, v = film_coordinates(oracle_mod, W, H, seed)
        o, d = _rays(oracle, u, v)
        h = oracle.trace(o, d).reshape(H, W)
        s = samples[f]
        s["d"], s["t"], s["u"], s["v"] = d, h["t"], h["u"], h["v"]
        s["instance"], s["primitive"] = h["instance"], h["primitive"]
        miss = h["t"] < 0
        for k in ("u", "v", "instance", "primitive"):
            s[k][miss] = 0
        origin[f], uv[f, :, :, 0], uv[f, :, :, 1] = o, u, v
        if edges:
            for du in (-DELTA, DELTA):
                for dv in (-DELTA, DELTA):
                    oo, dd = _rays(oracle, u + np.float32(du), v + np.float32(dv))
                    edge[f] |= ~_same(oracle.trace(oo, dd).reshape(H, W), h)
    return {"samples": samples, "origin": origin, "uv": uv, "edge": edge}


def crafted(ts, ids, d=(0.0, 0.0, 1.0)):
    """A (n, 1, 1) sample array for one pixel: hit distances `ts` (-1: a miss) with instance = primitive = `ids`."""
    s = np.zeros((len(ts), 1, 1), abi.PRIMARY_HIT_DTYPE)
    s["t"][:, 0, 0] = ts
    s["d"][:, 0, 0] = d
    s["instance"][:, 0, 0] = s["primitive"][:, 0, 0] = ids
    return s


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------------------------------
SCENES = ("cornell", "metal+spheres", "matte-deep+emitter", "matte+emissive-mesh", "metal-deep+spheres+sun", "fog")
VOLPATH = ("fog",)
FIRST, FRAMES = 3, 5            # the frames of the GPU tests: 3 .. 7
OTHER_SCENE, OTHER_FRAMES = "matte-deep+emitter", 16  # frames 3 .. 18 with ids="primitive": the reference reaches `other` and four filled slots
_cache = {}


def scene(name):
    import kernel_matrix as km
    return km.BY_NAME[name].build()


def reference(name):
    """reference_samples of frames FIRST .. (OTHER_FRAMES of them for OTHER_SCENE, FRAMES for the others), computed once per process."""
    if name not in _cache:
        from oracle import oracle as oracle_mod
        s = scene(name)
        o = oracle_mod.Oracle(s)
        _cache[name] = reference_samples(oracle_mod, o, s.xres if hasattr(s, "xres") else o.xres, o.yres, FIRST,
                                         OTHER_FRAMES if name == OTHER_SCENE else FRAMES)
    return _cache[name]


def first_frames(ref, n):
    """The first n frames of a reference_samples result."""
    return {k: v[:n] for k, v in ref.items()}

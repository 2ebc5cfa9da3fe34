"""GPU: the occlusion pass (rene_occlusion, rene_occlusion_samples; include/rene_hip.h) on the catalogue scenes of tests/kernel_matrix.py at
77 x 45, frames 3 .. 7, one and three rays per sample -- its records against the numpy restatement of the header (tests/occlusion_reference.py)
applied to its own samples, bit for bit; its verdicts against rene_trace; its random stream against the oracle's generator and its first hits
against rene_primary_hits; its directions against fp64; its normal against a rendered frame's first-hit normal layer; three scenes whose
occlusion is known in closed form; the context untouched; tile shards, caller-owned tensors, adaptive contexts; the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gbuffer_reference as gr
import kernel_matrix as km
import occlusion_reference as oref
from conftest import GOLDEN, ROOT
from gbuffer_reference import _assert_records_equal, _bits
from rene_amd import abi, api, glam, loader, scenes
from rene_amd.scene import Scene

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
FIRST, FRAMES = gr.FIRST, gr.FRAMES
FAR, SHORT = 1e5, 0.35  # the whole scene, and a radius inside the rooms: both verdicts occur
SETTINGS = ((1, SHORT), (3, SHORT), (3, FAR))  # (rays, radius)
_device = {}


def device(name):
    """The scene, a context on it and its own primary hits of frames FIRST .. (FRAMES of them), once per process."""
    if name not in _device:
        s = gr.scene(name)
        r = api.Renderer(s)
        _device[name] = {"scene": s, "r": r, "hits": r.primary_hits(FIRST, FRAMES), "origin": gr.camera_origin(s), "samples": {}}
    return _device[name]


def samples(name, rays, radius):
    """The context's own occlusion samples of frames FIRST .. under (rays, radius), once per process: (FRAMES, rays, H, W)."""
    d = device(name)
    if (rays, radius) not in d["samples"]:
        d["samples"][rays, radius] = d["r"].occlusion_samples(FIRST, FRAMES, rays, radius)
    return d["samples"][rays, radius]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for d in _device.values():
        d["r"].close()
    _device.clear()


@pytest.mark.parametrize("rays,radius", SETTINGS)
@pytest.mark.parametrize("name", gr.SCENES)
def test_records_are_the_restatement_of_the_own_samples(name, rays, radius):
    """occlusion(3, 5) and occlusion(3, 1) equal the numpy restatement applied to occlusion_samples: every field of every pixel, bit for bit."""
    d = device(name)
    s = samples(name, rays, radius)
    assert s.shape == (FRAMES, rays, km.H, km.W)
    for n in (FRAMES, 1):
        got = d["r"].occlusion(FIRST, n, rays, radius)
        assert got.shape == (km.H, km.W) and (got["n"] == n).all() and not got["reserved"].any()
        _assert_records_equal(got, oref.aggregate(s[:n]), (name, rays, radius, n))
    cast = got["rays"].sum()
    assert cast > 0.3 * km.H * km.W * rays and (got["rays"] == got["hits"] * rays).all()  # (no normal of these scenes is degenerate)
    if radius == SHORT:
        assert 0 < got["occluded"].sum() < cast  # both verdicts occur


@pytest.mark.parametrize("rays,radius", SETTINGS)
@pytest.mark.parametrize("name", gr.SCENES)
def test_verdicts_are_rene_traces(name, rays, radius):
    """For every ray cast, Renderer.trace(p, w, 0.001, radius) reports a hit exactly where the sample is occluded: no tolerance, no exclusions (a
    closest hit exists iff any hit does)."""
    flat = samples(name, rays, radius).reshape(-1)
    cast = flat[(flat["state"] == oref.OPEN) | (flat["state"] == oref.OCCLUDED)]
    assert len(cast) > 0.3 * len(flat) and (flat["state"] <= oref.NO_RAY).all()
    tr = device(name)["r"].trace(cast["p"], cast["w"], 0.001, radius)
    bad = (tr["t"] >= 0) != (cast["state"] == oref.OCCLUDED)
    assert not bad.any(), (name, rays, radius, int(bad.sum()), len(cast))


@pytest.mark.parametrize("name", gr.SCENES)
def test_the_stream_and_the_first_hit(name, oracle_mod):
    """r1 and r2 of ray k are draws 2 + 2 k and 3 + 2 k of the pixel's generator under the frame's seed (0 and 1 are the jitter); a miss exactly
    where primary_hits reports one; p within the project's 5e-5 (1 + |p|) of o + t d."""
    d = device(name)
    rays = 3
    s = samples(name, rays, FAR)
    hits = d["hits"]
    assert np.array_equal(s["state"] == oref.MISS, np.broadcast_to((hits["t"] < 0)[:, None], s.shape))
    assert (s["state"][:, 0:1] == oref.MISS).tobytes() == (s["state"][:, 1:2] == oref.MISS).tobytes()
    zero = s[s["state"] == oref.MISS]
    assert zero.tobytes() == bytes(48 * len(zero))  # everything else is 0
    seeds = api.frame_seeds(abi.DEFAULT_SEED, FIRST, FRAMES)
    want = np.zeros((FRAMES, rays, km.H, km.W, 2), np.float32)
    for f, seed in enumerate(seeds):
        for row in range(km.H):
            y = km.H - 1 - row
            for x in range(km.W):
                draws = oracle_mod.pcg_f32(((y * km.W + x) ^ int(seed)) & 0xFFFFFFFF, 2 + 2 * rays)
                want[f, :, row, x] = np.asarray(draws[2:]).reshape(rays, 2)
    cast = (s["state"] == oref.OPEN) | (s["state"] == oref.OCCLUDED)
    assert cast.mean() > 0.3
    assert np.array_equal(_bits(s["r1"])[cast], _bits(want[..., 0])[cast]) and np.array_equal(_bits(s["r2"])[cast], _bits(want[..., 1])[cast])
    p = d["origin"].astype(np.float64) + hits["t"].astype(np.float64)[..., None] * hits["d"].astype(np.float64)
    got = s["p"].astype(np.float64)
    for k in range(rays):
        hit = s["state"][:, k] != oref.MISS
        err = np.abs(got[:, k][hit] - p[hit]) / (5e-5 * (1 + np.abs(p[hit])))
        assert (err <= 1).all(), (name, k, float(err.max()))
        assert np.array_equal(_bits(s["p"][:, k]), _bits(s["p"][:, 0])) and np.array_equal(_bits(s["n"][:, k]), _bits(s["n"][:, 0]))
    print(name, "largest position error in units of the bound", float(err.max()))


@pytest.mark.parametrize("name", gr.SCENES)
def test_directions_against_fp64(name):
    """|w - direction(n, r1, r2)| <= 2^-10 per component: bsdf_reference.py's budget of 2^-11 absolute on the hardware sine and cosine, through a
    frame whose rows are unit vectors (a component of w moves by at most sqrt(2) 2^-11).  A wrong stream, swapped draws or a wrong axis moves w by
    tenths.  |n| is within 1e-5 of 1 and n faces the viewer."""
    d = device(name)
    s = samples(name, 3, FAR)
    cast = (s["state"] == oref.OPEN) | (s["state"] == oref.OCCLUDED)
    c = s[cast]
    err = np.abs(c["w"].astype(np.float64) - oref.direction(c["n"], c["r1"], c["r2"]))
    print(name, "largest direction error", err.max(), "of", 2.0 ** -10)
    assert err.max() <= 2.0 ** -10
    n = c["n"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() <= 1e-5
    dirs = np.broadcast_to(d["hits"]["d"][:, None], s.shape + (3,))[cast].astype(np.float64)
    assert ((n * dirs).sum(-1) <= 1e-6).all()
    assert ((c["w"].astype(np.float64) * n).sum(-1) >= -2.0 ** -9).all()  # the hemisphere of n


@pytest.mark.parametrize("name", [n for n in gr.SCENES if n not in gr.VOLPATH])
def test_the_normal_is_the_renders(name, oracle_mod):
    """Frame 7 rendered alone on a fresh context: off that frame's edge samples, n is + or - the fp64-normalised first-hit normal layer within 1e-5."""
    f = 7
    edge = gr.reference(name)["edge"][f - FIRST]
    with api.Renderer(gr.scene(name)) as r:
        r.render(f, 1)
        normal = r.download(abi.LAYER_NORMAL)[..., :3].astype(np.float64)
        s = r.occlusion_samples(f, 1, 1, FAR)[0, 0]
    seen = (normal != 0).any(-1)
    keep = seen & ~edge
    assert 0.3 < keep.mean() and (s["state"][keep] != oref.MISS).all() and (s["state"][~seen & ~edge] == oref.MISS).all()
    unit = normal[keep] / np.linalg.norm(normal[keep], axis=-1, keepdims=True)
    n = s["n"][keep].astype(np.float64)
    err = np.minimum(np.abs(n - unit).max(-1), np.abs(n + unit).max(-1))
    print(name, "largest normal error", err.max())
    assert err.max() <= 1e-5


# ---- scenes whose occlusion is known in closed form ------------------------------------------------------------------------------------------------
def _floor_from_above(wall=False):
    """A floor quad at y = 0 seen from (0, 5, 0) straight down; `wall`: the floor ends at x = 3 under a wall that stands on it, 10^4 high and
    2 10^4 long -- more than 1000 times the 6 units the film's floor points are away from it at most."""
    s = Scene.new()
    s.set_camera(glam.look_at_lh((0.0, 5.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), 38.0, km.W, km.H)
    m = s.add_matte((0.5, 0.5, 0.5))
    x1 = 3.0 if wall else 10.0
    s.add_triangle_mesh(scenes._quad([-10, 0, -10, -10, 0, 10, x1, 0, 10, x1, 0, -10], (0, 1, 0)), m)
    if wall:
        s.add_triangle_mesh(scenes._quad([3, 0, -1e4, 3, 1e4, -1e4, 3, 1e4, 1e4, 3, 0, 1e4], (-1, 0, 0)), m)
    return s


def test_a_lone_floor_is_open_and_its_directions_are_cosine_distributed():
    """occluded == 0 everywhere; over all N rays the mean of w . n is 2 / 3 +- 5 sqrt(1 / (18 N)) (E cos = 2 / 3, E cos^2 = 1 / 2 under the cosine
    density; a uniform hemisphere gives 1 / 2) and each tangential mean is 0 +- 5 sqrt(1 / (4 N)) (E x^2 = 1 / 4)."""
    rays = 3
    with api.Renderer(_floor_from_above()) as r:
        rec = r.occlusion(FIRST, FRAMES, rays, FAR)
        s = r.occlusion_samples(FIRST, FRAMES, rays, FAR)
    assert (rec["hits"] == FRAMES).all() and (rec["rays"] == FRAMES * rays).all() and not rec["occluded"].any()
    assert (api.occlusion_ao(rec) == 1).all() and (s["state"] == oref.OPEN).all()
    assert np.abs(s["n"].reshape(-1, 3) - np.float32([0, 1, 0])).max() <= 1e-6
    w = s["w"].reshape(-1, 3).astype(np.float64)
    N = len(w)
    print("mean w:", w.mean(0), "N", N)
    assert abs(w[:, 1].mean() - 2.0 / 3.0) <= 5 * np.sqrt(1 / (18 * N))
    assert abs(w[:, 0].mean()) <= 5 * np.sqrt(1 / (4 * N)) and abs(w[:, 2].mean()) <= 5 * np.sqrt(1 / (4 * N))
    assert (w[:, 1] > 0).all() and (api.occlusion_bent(rec)[..., 1] > 0).all()  # z = sqrt(1 - r2) >= 2^-12: every direction, and so their sum, leans to n


def test_inside_a_closed_cube_everything_is_occluded():
    s = Scene.new()
    s.set_camera(glam.look_at_lh((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)), 38.0, km.W, km.H)
    s.add_triangle_mesh(scenes._aabb((-1, -1, -1), (1, 1, 1)), s.add_matte((0.5, 0.5, 0.5)))
    with api.Renderer(s) as r:
        rec = r.occlusion(FIRST, FRAMES, 3, FAR)
    assert (rec["hits"] == FRAMES).all() and (rec["rays"] == 3 * FRAMES).all() and (rec["occluded"] == rec["rays"]).all()
    assert not rec["bent_sum"].any() and (api.occlusion_ao(rec) == 0).all() and not api.occlusion_bent(rec).any()


def test_a_floor_next_to_a_large_wall_is_half_occluded():
    """The floor's rays whose direction leans to the wall hit it, but for a share of the order of the 1 / 1000 the wall is short of a half space:
    the mean occlusion of the floor's N rays is 1 / 2 +- (5 sqrt(1 / (4 N)) + 0.005)."""
    with api.Renderer(_floor_from_above(wall=True)) as r:
        s = r.occlusion_samples(FIRST, FRAMES, 3, FAR).reshape(-1)
    floor = s[(s["state"] != oref.MISS) & (s["n"][:, 1] > 0.999) & (np.abs(s["p"][:, 1]) <= 1e-6)]
    N = len(floor)
    assert N > 0.5 * len(s) and (3 - floor["p"][:, 0]).max() <= 6.5 and (floor["p"][:, 0] <= 3).all()
    mean = (floor["state"] == oref.OCCLUDED).mean()
    print("mean occlusion", mean, "N", N)
    assert abs(mean - 0.5) <= 5 * np.sqrt(1 / (4 * N)) + 0.005
    assert ((floor["state"] == oref.OCCLUDED) <= (floor["w"][:, 0] > 0)).all()  # only a ray that leans to the wall can hit it


# ---- the context, shards, tensors, adaptive contexts, the command line ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "matte-deep+emitter"])
def test_the_context_is_untouched(name):
    def job(between):
        with api.Renderer(gr.scene(name), flags=abi.FLAG_COUNTERS) as r:
            r.render(0, 8)
            if between:
                r.occlusion(2, 7, 3, SHORT)
                r.occlusion_samples(1, 3, 2, FAR)
                r.occlusion(0, 16)
            r.render(8, 8)
            layers = [r.download(l) for l in range(3)]
            st = r.stats()
        return layers, {k: getattr(st, k) for k in ("rays_closest", "rays_shadow", "rays_emitter", "paths", "bounces", "hits", "adds", "frames")}
    (la, sa), (lb, sb) = job(True), job(False)
    for a, b in zip(la, lb):
        assert np.array_equal(a, b)
    assert sa == sb and sa["frames"] == 16 and sa["rays_closest"] > 0


def test_tile_shards_merge_to_the_unsharded_records():
    s = scenes.cornell_box(100, 70)  # 4 x 3 tiles
    with api.Renderer(s) as r:
        whole = r.occlusion(FIRST, FRAMES, 3, SHORT)
    parts = []
    for rank in range(3):
        with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            parts.append(r.occlusion(FIRST, FRAMES, 3, SHORT))
            smp = r.occlusion_samples(FIRST, 1, 2, SHORT)
        own = gr.owned_mask(100, 70, rank, 3)
        assert parts[-1][~own].tobytes() == bytes(32 * int((~own).sum())) and (parts[-1]["n"][own] == FRAMES).all()
        assert smp[:, :, ~own].tobytes() == bytes(48 * 2 * int((~own).sum()))
    assert api.occlusion_merge(parts).tobytes() == whole.tobytes()
    assert (whole["n"] == FRAMES).all() and (whole["hits"] > 0).mean() > 0.5 and 0 < whole["occluded"].sum() < whole["rays"].sum()


def test_occlusion_into_a_tensor_and_the_librarys_buffer():
    import torch
    r = device("cornell")["r"]
    want = r.occlusion(FIRST, FRAMES, 3, SHORT)
    ptr, n = r.occlusion_buffer()
    assert ptr and n == km.W * km.H * 32 == api.occlusion_bytes(km.W, km.H)
    t = torch.full((km.H, km.W, 32), 0xAB, dtype=torch.uint8, device="cuda")
    assert r.occlusion_into(t, FIRST, FRAMES, 3, SHORT) is t
    r.sync()
    assert t.cpu().numpy().tobytes() == want.tobytes()
    t32 = torch.full((km.H, km.W, 8), -1, dtype=torch.int32, device="cuda")
    assert r.occlusion_into(t32, FIRST, FRAMES, 3, SHORT) is t32
    r.sync()
    assert t32.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        r.occlusion_into(torch.zeros(km.H * km.W * 32 - 32, dtype=torch.uint8, device="cuda"), FIRST, FRAMES)
    with pytest.raises(ValueError):
        r.occlusion_into(torch.zeros(km.H * km.W * 32, dtype=torch.int32, device="cuda"), FIRST, FRAMES)  # four times the bytes
    with pytest.raises(TypeError):
        r.occlusion_into(torch.zeros(km.H * km.W * 8, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        r.occlusion_into(torch.zeros(km.H * km.W * 32, dtype=torch.uint8), FIRST, FRAMES)  # host memory
    # the library's own refusals: a destination that is too small, one that is misaligned
    p = api.occlusion_params_default()
    for dst, size in ((t.data_ptr(), t.numel() - 1), (t.data_ptr() + 4, t.numel() - 4)):
        with pytest.raises(api.ReneError) as e:
            api._check(api.lib().rene_occlusion(r._h, C.byref(p), C.c_void_p(dst), size))
        assert e.value.code == -1
    one = np.zeros(1, abi.OCCLUSION_SAMPLE_DTYPE)  # more than 2^22 records: refused before the destination is looked at
    p.n_frames, p.rays = 65536, 64
    assert api.lib().rene_occlusion_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"2^22" in api.lib().rene_last_error()
    p.n_frames, p.rays = 2, 2
    assert api.lib().rene_occlusion_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"smaller" in api.lib().rene_last_error()


def test_an_adaptive_context_gives_the_even_contexts_records():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r:
        even = r.occlusion(FIRST, FRAMES, 3, SHORT)
    with api.Renderer(s) as r:
        r.render(0, 8)
        active = np.indices((3, 4)).sum(0) % 2  # half of the tiles go on
        r.set_active_tiles(active)
        r.render(8, 8)
        assert r.occlusion(FIRST, FRAMES, 3, SHORT).tobytes() == even.tobytes()
        assert sorted(set(r.tile_frames().reshape(-1).tolist())) == [8, 16]  # (the mask was in force, and still is)


def _read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = map(int, f.readline().split())
        assert float(f.readline()) == -1.0
        ch = {b"PF": 3, b"Pf": 1}[kind]
        a = np.frombuffer(f.read(), "<f4").reshape(h, w, ch)
    return a[::-1]  # bottom row first in the file


def test_the_command_line_writes_the_three_files(hip_lib, tmp_path):
    path = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    W, H = 100, 70
    p = subprocess.run([CLI, path, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", "--ao", "a", "--ao-frames", "4", "--ao-rays", "3",
                        "--ao-radius", "0.35"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.ao.pfm", "a.ao.png", "a.bent.pfm", "o.png"]
    loaded = loader.load_pbrt(path)
    desc = loaded.desc  # the command line's override of the Film size: the projection's x axis rescaled to the new aspect, in fp32
    ratio = np.float32(np.float32(W) / np.float32(H)) / np.float32(np.float32(desc.xresolution) / np.float32(desc.yresolution))
    desc.uniform.projection_inv[0] = np.float32(np.float32(desc.uniform.projection_inv[0]) * ratio)
    desc.xresolution, desc.yresolution = W, H
    loaded.xres, loaded.yres = W, H
    with api.Renderer(loaded) as r:
        rec = r.occlusion(0, 4, 3, 0.35)
    ao = api.occlusion_ao(rec)
    assert _read_pfm(tmp_path / "a.ao.pfm")[..., 0].tobytes() == ao.tobytes()
    assert _read_pfm(tmp_path / "a.bent.pfm").tobytes() == api.occlusion_bent(rec).tobytes()
    assert (rec["hits"] > 0).mean() > 0.5 and 0 < rec["occluded"].sum() < rec["rays"].sum()
    png = open(tmp_path / "a.ao.png", "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[16:26] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + b"\x08\x00"  # 8-bit grey
    import zlib
    at, idat = 8, b""
    while at < len(png):
        n, kind = int.from_bytes(png[at:at + 4], "big"), png[at + 4:at + 8]
        if kind == b"IDAT":
            idat += png[at + 8:at + 8 + n]
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, W + 1)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:], np.floor(np.float32(255) * ao + np.float32(0.5)).astype(np.uint8))

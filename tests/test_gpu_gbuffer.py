"""GPU: the geometry pass (rene_gbuffer, rene_primary_hits; include/rene_hip.h) on the catalogue scenes of tests/kernel_matrix.py at 77 x 45 --
its samples against rene_trace (bit for bit), against the oracle's camera and against the fp64 reference; its records against the numpy
restatement of the header (tests/gbuffer_reference.py) applied to its own samples (bit for bit) and to the oracle's (off the edge samples); the
pass against a rendered frame's first-hit layer; the context untouched; tile shards, caller-owned tensors, adaptive contexts; the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gbuffer_reference as gr
import kernel_matrix as km
import transform_cases as tc
from conftest import GOLDEN, ROOT
from gbuffer_reference import _assert_records_equal, _bits
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
FIRST, FRAMES = gr.FIRST, gr.FRAMES
_device = {}


def device(name):
    """The scene, a context on it and its own samples of frames FIRST .. (FRAMES of them; OTHER_FRAMES for OTHER_SCENE), once per process."""
    if name not in _device:
        s = gr.scene(name)
        r = api.Renderer(s)
        n = gr.OTHER_FRAMES if name == gr.OTHER_SCENE else FRAMES
        _device[name] = {"scene": s, "r": r, "hits": r.primary_hits(FIRST, n), "origin": gr.camera_origin(s), "materials": gr.instance_materials(s)}
    return _device[name]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for d in _device.values():
        d["r"].close()
    _device.clear()


@pytest.mark.parametrize("name", gr.SCENES)
def test_samples_are_rene_traces_of_their_own_directions(name):
    """The same instantiation of the closest-hit query on the same operands: t, u, v, instance, primitive bit for bit."""
    d = device(name)
    h = d["hits"][:FRAMES]
    assert h.shape == (FRAMES, km.H, km.W)
    dirs = h["d"].reshape(-1, 3)
    tr = d["r"].trace(np.broadcast_to(d["origin"], dirs.shape), dirs)
    flat = h.reshape(-1)
    for k in ("t", "u", "v", "instance", "primitive"):
        bad = _bits(flat[k]) != _bits(tr[k])
        assert not bad.any(), (name, k, int(bad.sum()))
    hit = flat["t"] >= 0
    assert 0.3 < hit.mean() and len(np.unique(flat["instance"][hit])) >= 2  # (the fog scene: the medium's boundary box and the floor behind its open side)


@pytest.mark.parametrize("name", gr.SCENES)
def test_rays_are_the_oracles_camera_rays(name, oracle_mod):
    """Against Oracle.camera_ray at the reference's (u, v): 1e-5 per component -- a wrong stream, a swapped jitter, W for W - 1 or a pixel off
    by one moves a direction by about a pixel's angle, 1e-2 here; fp32 (qdiv's 2 ulp, two matrix products, rsq) by about 1e-6."""
    ref = gr.first_frames(gr.reference(name), FRAMES)
    err = np.abs(device(name)["hits"][:FRAMES]["d"].astype(np.float64) - ref["samples"]["d"])
    print(name, "largest direction error", err.max())
    assert err.max() <= 1e-5
    assert np.abs(ref["origin"] - device(name)["origin"]).max() <= 1e-6  # the origin of rene_primary_hit's rays: the translation column


@pytest.mark.parametrize("name", gr.SCENES)
def test_hits_against_the_fp64_reference_and_the_oracle(name, oracle_mod):
    """The device's own directions -- the first and the last frame of the probe: the brute force in fp64 takes a second per frame on the deep
    scenes -- through transform_cases.Reference and through Oracle.trace, both judged by transform_cases.compare_hits as it stands."""
    d = device(name)
    h = d["hits"][:FRAMES]
    two = h[[0, FRAMES - 1]].reshape(-1)
    o2 = np.broadcast_to(d["origin"], (len(two), 3))
    ref = tc.Reference(d["scene"]).trace(o2, two["d"])
    n = tc.compare_hits(two, ref, name + " device")
    print(name, n, "of", len(two), "rays judged,", int(ref["grazing"].sum()), "grazing")
    assert n >= 0.98 * len(two)
    ora = oracle_mod.Oracle(d["scene"])
    ho = ora.trace(o2, two["d"])
    assert tc.compare_hits(ho, ref, name + " oracle") == n


@pytest.mark.parametrize("ids", gr.ID_NAMES)
@pytest.mark.parametrize("name", gr.SCENES)
def test_records_are_the_restatement_of_the_own_samples(name, ids):
    """gbuffer(3, 5) and gbuffer(3, 1) equal the numpy restatement applied to primary_hits: every field of every pixel, bit for bit."""
    d = device(name)
    for n in (FRAMES, 1):
        got = d["r"].gbuffer(FIRST, n, ids=ids)
        assert got.shape == (km.H, km.W) and (got["n"] == n).all()
        _assert_records_equal(got, gr.aggregate(d["hits"][:n], d["origin"], ids, d["materials"]), (name, ids, n))


def test_the_other_path_and_four_filled_slots():
    """matte-deep+emitter, ids="primitive", 16 frames: the inputs whose reference records reach `other` and four filled slots
    (test_gbuffer_reference.py)."""
    d = device(gr.OTHER_SCENE)
    got = d["r"].gbuffer(FIRST, gr.OTHER_FRAMES, ids="primitive")
    assert (got["other"] > 0).any() and (((got["count"] > 0).sum(-1) == 4) & (got["other"] == 0)).any()
    _assert_records_equal(got, gr.aggregate(d["hits"], d["origin"], "primitive"), "other")


@pytest.mark.parametrize("name", gr.SCENES)
def test_records_against_the_oracles(name, oracle_mod):
    """The sample generator's records are the reference.  On every pixel none of whose samples is an edge sample: hits, id[], count[] and other
    are equal (all three id sources); depth_sum, depth_min and position_sum within 5e-5 n (1 + |ref|), the project's margin for t, summed."""
    d = device(name)
    ref = gr.first_frames(gr.reference(name), FRAMES)
    keep = ~ref["edge"].any(0)
    assert keep.mean() >= 1 - FRAMES * gr.EDGE_CAP
    for ids in gr.ID_NAMES:
        got = d["r"].gbuffer(FIRST, FRAMES, ids=ids)
        want = gr.aggregate(ref["samples"], ref["origin"], ids, d["materials"])
        for k in ("hits", "n", "other", "id", "count"):
            bad = (got[k] != want[k]).reshape(km.H, km.W, -1).any(-1) & keep
            assert not bad.any(), (name, ids, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    for k in ("depth_sum", "depth_min", "position_sum"):
        g, w = got[k][keep].astype(np.float64), want[k][keep].astype(np.float64)
        nothing = ~np.isfinite(w)  # depth_min where nothing hit: +inf on both sides
        assert np.array_equal(g[nothing], w[nothing])
        err = np.abs(g[~nothing] - w[~nothing]) / (5e-5 * FRAMES * (1 + np.abs(w[~nothing])))
        print(name, k, "largest error in units of the bound", err.max() if err.size else 0.0)
        assert (err <= 1).all(), (name, k, float(err.max()))


@pytest.mark.parametrize("name", [n for n in gr.SCENES if n not in gr.VOLPATH])
def test_the_pass_is_the_renders_first_hit(name, oracle_mod):
    """One rendered frame f = 7 on a fresh context: off that frame's edge samples, hits == 1 exactly where the first-hit normal layer is non-zero."""
    f = 7
    edge = gr.reference(name)["edge"][f - FIRST]
    with api.Renderer(gr.scene(name)) as r:
        r.render(f, 1)
        normal = r.download(abi.LAYER_NORMAL)
        rec = r.gbuffer(f, 1)
    seen = (normal != 0).any(-1)
    assert 0.3 < seen.mean()
    bad = ((rec["hits"] == 1) != seen) & ~edge
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("name", ["cornell", "matte-deep+emitter"])
def test_the_context_is_untouched(name):
    def job(between):
        with api.Renderer(gr.scene(name), flags=abi.FLAG_COUNTERS) as r:
            r.render(0, 8)
            if between:
                r.gbuffer(2, 7, ids="material")
                r.primary_hits(1, 3)
                r.gbuffer(0, 16)
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
        whole = r.gbuffer(FIRST, FRAMES, ids="primitive")
    parts = []
    for rank in range(3):
        with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            parts.append(r.gbuffer(FIRST, FRAMES, ids="primitive"))
        own = gr.owned_mask(100, 70, rank, 3)
        assert parts[-1][~own].tobytes() == bytes(64 * int((~own).sum())) and (parts[-1]["n"][own] == FRAMES).all()
    assert api.gbuffer_merge(parts).tobytes() == whole.tobytes()
    assert (whole["n"] == FRAMES).all() and (whole["hits"] > 0).mean() > 0.5


def test_gbuffer_into_a_tensor_and_the_librarys_buffer():
    import torch
    d = device("cornell")
    r = d["r"]
    want = r.gbuffer(FIRST, FRAMES)
    ptr, n = r.gbuffer_buffer()
    assert ptr and n == km.W * km.H * 64 == api.gbuffer_bytes(km.W, km.H)
    t = torch.full((km.H, km.W, 64), 0xAB, dtype=torch.uint8, device="cuda")
    assert r.gbuffer_into(t, FIRST, FRAMES) is t
    r.sync()
    assert t.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        r.gbuffer_into(torch.zeros(km.H * km.W * 64 - 64, dtype=torch.uint8, device="cuda"), FIRST, FRAMES)
    with pytest.raises(TypeError):
        r.gbuffer_into(torch.zeros(km.H * km.W * 16, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        r.gbuffer_into(torch.zeros(km.H * km.W * 64, dtype=torch.uint8), FIRST, FRAMES)  # host memory
    # the library's own refusals: a destination that is too small, one that is misaligned
    p = api.gbuffer_params_default()
    for dst, size in ((t.data_ptr(), t.numel() - 1), (t.data_ptr() + 4, t.numel() - 4)):
        with pytest.raises(api.ReneError) as e:
            api._check(api.lib().rene_gbuffer(r._h, C.byref(p), C.c_void_p(dst), size))
        assert e.value.code == -1
    one = np.zeros(1, abi.PRIMARY_HIT_DTYPE)  # more than 2^24 samples: refused before the destination is looked at
    assert api.lib().rene_primary_hits(r._h, 0, 65536, one.ctypes.data_as(C.c_void_p), 1) == -1 and b"2^24" in api.lib().rene_last_error()


def test_an_adaptive_context_gives_the_even_contexts_records():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r:
        even = r.gbuffer(FIRST, FRAMES)
    with api.Renderer(s) as r:
        r.render(0, 8)
        active = np.indices((3, 4)).sum(0) % 2  # half of the tiles go on
        r.set_active_tiles(active)
        r.render(8, 8)
        assert r.gbuffer(FIRST, FRAMES).tobytes() == even.tobytes()
        assert sorted(set(r.tile_frames().reshape(-1).tolist())) == [8, 16]  # (the mask was in force, and still is)


def _read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = map(int, f.readline().split())
        assert float(f.readline()) == -1.0
        ch = {b"PF": 3, b"Pf": 1}[kind]
        a = np.frombuffer(f.read(), "<f4").reshape(h, w, ch)
    return a[::-1]  # bottom row first in the file


def test_the_command_line_writes_the_four_files(hip_lib, tmp_path):
    path = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    W, H = 100, 70
    p = subprocess.run([CLI, path, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", "--gbuffer", "g", "--gbuffer-frames", "4"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == ["g.coverage.pfm", "g.depth.pfm", "g.id.png", "g.position.pfm", "o.png"]
    loaded = loader.load_pbrt(path)
    desc = loaded.desc  # the command line's override of the Film size: the projection's x axis rescaled to the new aspect, in fp32
    ratio = np.float32(np.float32(W) / np.float32(H)) / np.float32(np.float32(desc.xresolution) / np.float32(desc.yresolution))
    desc.uniform.projection_inv[0] = np.float32(np.float32(desc.uniform.projection_inv[0]) * ratio)
    desc.xresolution, desc.yresolution = W, H
    loaded.xres, loaded.yres = W, H
    with api.Renderer(loaded) as r:
        rec = r.gbuffer(0, 4)
    depth = api.gbuffer_depth(rec)
    depth[rec["hits"] == 0] = 0  # the file holds 0 where nothing hit
    assert _read_pfm(tmp_path / "g.depth.pfm")[..., 0].tobytes() == depth.tobytes()
    assert _read_pfm(tmp_path / "g.coverage.pfm")[..., 0].tobytes() == api.gbuffer_coverage(rec).tobytes()
    assert _read_pfm(tmp_path / "g.position.pfm").tobytes() == api.gbuffer_position(rec).tobytes()
    assert (rec["hits"] > 0).mean() > 0.5 and open(tmp_path / "g.id.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n"

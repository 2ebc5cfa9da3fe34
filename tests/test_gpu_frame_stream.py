"""The frame-wide sample stream as a per-launch table (device_scene.h, FRAME_STREAM_*; rene_frame_stream_probe).

The Matte small-scene kernels no longer draw the reference's frame-wide generator (quirk Q3) in every lane: a one-thread-per-frame kernel walks
it before the launch and the render kernel reads entry [launch frame][depth].  What is checked:

* the table's contents against a numpy restatement of the stream, replayed from the frame seeds with PCG32si (pinned by
  tests/golden/pcg32si_kat.json, checked here without a GPU): coin decisions and roulette numbers EQUAL at every depth of every frame -- the
  coin at every later depth being right is what proves the stream position, i.e. that the kernel draws what the integrator draws, in its order;
* images: Cornell and Cornell + a distant light, with and without AOVs, bit-equal to layers recorded with the library of the commit before the
  table existed (tests/golden/make_frame_stream_golden.py), in one call, in two calls of 9 + 7 frames (a table whose first frame is not 0) and
  as the sum of a 2-rank tile shard."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rene_amd import abi, api, scenes
from rene_amd.scene import TriangleMesh

M32 = 0xFFFFFFFF
DEPTHS = 50
U = 2.0 ** -24  # unit roundoff of fp32


# ---- PCG32si, rene-shader/src/rand.rs:4-52, in Python integers -------------------------------------------------------------------------
class Pcg:
    def __init__(self, seed):
        self.s = seed & M32
        self.step()
        self.s = (self.s + seed) & M32
        self.step()

    def step(self):
        self.s = (self.s * 747796405 + 2891336453) & M32

    def u32(self):
        s = self.s
        self.step()
        word = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & M32
        return (word >> 22) ^ word

    def f32(self):
        return np.float32(self.u32() >> 8) * np.float32(U)  # exact: a 24-bit integer times a power of two


def test_restatement_of_pcg32si_matches_the_known_answers():
    kat = json.load(open(os.path.join(GOLDEN, "pcg32si_kat.json")))
    assert len(kat) > 0
    for seed, rec in kat.items():  # {seed: {"state_after_new": ..., "u32": [...]}}
        g = Pcg(int(seed))
        assert g.s == int(rec["state_after_new"]), seed
        assert [g.u32() for _ in rec["u32"]] == [int(v) for v in rec["u32"]], seed


# ---- the stream of one frame, restated (lib.rs:274-324, 345-354; surface_sample.rs:69-117) --------------------------------------------
def restate_frame(seed, emitters):
    """emitters: [(vertices float32 [nv][3] in world space, indices [ntri][3])] in emit-object order.  Returns coin [50] bool, rr [50] float32
    (0 where none is drawn), on_light [50][3] float32 and per component the sum of the three terms' magnitudes (the error bound's scale)."""
    fw = Pcg(seed)
    coin, rr = np.zeros(DEPTHS, bool), np.zeros(DEPTHS, np.float32)
    on, scale = np.zeros((DEPTHS, 3), np.float32), np.zeros((DEPTHS, 3), np.float64)
    one = np.float32(1)
    for d in range(DEPTHS):
        if emitters and fw.f32() > np.float32(0.5):
            coin[d] = True
            v, idx = emitters[fw.u32() % len(emitters)]
            p0, p1, p2 = (v[k] for k in idx[fw.u32() % len(idx)])  # Q6
            r, s = fw.f32(), fw.f32()
            if r + s > one:
                r, s = one - r, one - s
            b0 = one - r - s
            on[d] = p0 * b0 + p1 * r + p2 * s  # fp32 throughout, every operation rounded
            scale[d] = np.abs(p0 * b0).astype(np.float64) + np.abs(p1 * r) + np.abs(p2 * s)
        if d > 12:
            rr[d] = fw.f32()
    return coin, rr, on, scale


def quad(p, n):
    return TriangleMesh.from_arrays(p, [0, 1, 2, 0, 2, 3], normals=[n] * 4, uvs=[0, 0, 1, 0, 1, 1, 0, 1])


CORNELL_LIGHT = [-0.24, 1.98, -0.22, 0.23, 1.98, -0.22, 0.23, 1.98, 0.16, -0.24, 1.98, 0.16]


def many_emitters():
    """Cornell + two more emitters: three emit objects (the `x % n` arm of umod, n = 3) of 2, 2 and 3 triangles (n = 3 again, on the primitive)."""
    s = scenes.cornell_box(40, 40)
    extra = [(quad([-0.9, 0.3, -0.99, -0.5, 0.3, -0.99, -0.5, 0.8, -0.99, -0.9, 0.8, -0.99], (0, 0, 1)), (3.0, 1.0, 0.5)),
             (TriangleMesh.from_arrays([0.5, 1.2, -0.99, 0.9, 1.2, -0.99, 0.95, 1.5, -0.99, 0.7, 1.8, -0.99, 0.45, 1.5, -0.99],
                                       [0, 1, 2, 0, 2, 3, 0, 3, 4], normals=[(0, 0, 1)] * 5, uvs=[0, 0] * 5), (0.5, 2.0, 4.0))]
    meshes = [(np.asarray(CORNELL_LIGHT, np.float32).reshape(-1, 3), np.asarray([0, 1, 2, 0, 2, 3]).reshape(-1, 3))]
    for mesh, L in extra:
        s.add_triangle_mesh(mesh, s.add_matte((0.0, 0.0, 0.0)), area_light=s.add_area_light_diffuse(L))
        meshes.append((np.ascontiguousarray(mesh.vertices[:, 0:3], np.float32), np.asarray(mesh.indices).reshape(-1, 3)))
    return s, meshes


def no_emitters():
    """The room lit by a distant light only: nobody draws the coin, the table holds the roulette numbers alone."""
    s = scenes.cornell_box(40, 40)
    s.instances.pop()  # the light quad (the last instance)
    s.add_light_distant((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))
    return s, []


def cornell_table_scene():
    return scenes.cornell_box(40, 40), [(np.asarray(CORNELL_LIGHT, np.float32).reshape(-1, 3), np.asarray([0, 1, 2, 0, 2, 3]).reshape(-1, 3))]


TABLE_CASES = {"cornell": cornell_table_scene, "many-emitters": many_emitters, "no-emitters": no_emitters}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_table_equals_the_restated_stream(name):
    scene, emitters = TABLE_CASES[name]()
    info = api.pack_info(scene).as_dict()
    assert info["features"] & abi.FEAT_SMALL and info["emit_object_len"] == len(emitters)
    seed, first, n = 0xC0FFEE, 1000, 96
    with api.Renderer(scene, seed=seed) as r:
        got = r.frame_stream_probe(first, n)
        again = r.frame_stream_probe(first + 5, 7)
    assert np.array_equal(got[5:12].view(np.uint32), again.view(np.uint32))  # an entry depends on its global frame alone
    bits = got[..., 3].view(np.uint32)
    seeds = api.frame_seeds(seed, first, n)
    worst, lights, worst_ulp = 0.0, 0, 0.0
    for i in range(n):
        coin, rr, on, scale = restate_frame(int(seeds[i]), emitters)
        assert np.array_equal(bits[i] >> 31 != 0, coin), (name, i)                              # the coin: equal, at every depth
        assert np.array_equal(bits[i] & 0x7FFFFFFF, rr.view(np.uint32)), (name, i)              # the roulette number: equal bits (0 up to depth 12)
        assert (got[i, ~coin, :3].view(np.uint32) == 0).all(), (name, i)                        # no point where none is sampled
        diff = np.abs(got[i, :, :3].astype(np.float64) - on.astype(np.float64))
        # on_light = p0 b0 + p1 r + p2 s: five rounded operations here, and the device may fuse a product into the sum that follows it.  Both
        # results are within gamma_3 = 3 u / (1 - 3 u) of the exact sum of the three (identical) products, relative to the sum of their
        # magnitudes (the textbook bound of a three-term sum of products, u = 2^-24) -- so they are within 6.000001 u of it of each other.
        # b0 = 1 - r - s has no product to fuse and is the same number on both sides.  Measured on an MI355X: 0 on all 2 438 points of every
        # case -- -ffp-contract=on fuses within one source expression, and the products and sums of `f3` are operator calls -- so the
        # bound is what a compiler that fused them would still be held to.
        assert (diff <= 6.000001 * U * scale).all(), (name, i, float((diff / np.maximum(scale, 1e-30)).max() / U))
        lights += int(coin.sum())
        if coin.any():
            worst = max(worst, float((diff[coin] / np.maximum(scale[coin], 1e-30)).max() / U))
            worst_ulp = max(worst_ulp, float((diff[coin] / np.spacing(np.abs(on[coin]).astype(np.float32) + np.float32(1e-30))).max()))
    print(f"{name}: {n} frames x {DEPTHS} depths, {lights} emitter points; largest on_light difference {worst:.3f} u of the terms' magnitudes "
          f"({worst_ulp:.2f} ulp of the value), bound 6 u")
    if emitters:
        assert DEPTHS * n * 0.4 < lights < DEPTHS * n * 0.6  # a fair coin
    else:
        assert lights == 0 and (bits[:, 13:] != 0).any()


# ---- images against the per-lane stream ----------------------------------------------------------------------------------------------
W, H, FRAMES, SPLIT = 48, 40, 16, 9


def golden_scene(name):
    s = scenes.cornell_box(W, H)
    if name == "cornell_sun":
        s.add_light_distant((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))
    return s


def layers(r):
    return np.stack([r.download(k) for k in range(3)])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", ["aov", "noaov"])
@pytest.mark.parametrize("name", ["cornell", "cornell_sun"])
def test_images_equal_the_per_lane_stream(name, flags):
    want = np.load(os.path.join(GOLDEN, "frame_stream_layers.npz"))[f"{name}_{flags}"]
    f = abi.FLAG_NO_AOV if flags == "noaov" else 0
    with api.Renderer(golden_scene(name), flags=f) as r:
        r.render(0, FRAMES)
        one = layers(r)
        r.reset()
        r.render(0, SPLIT)
        r.render(SPLIT, FRAMES - SPLIT)  # its table starts at frame 9
        two = layers(r)
    assert np.array_equal(one, want), (name, flags, float(np.abs(one - want).max()))
    assert np.array_equal(two, want), (name, flags, float(np.abs(two - want).max()))
    shards = np.zeros_like(want)
    for rank in range(2):
        with api.Renderer(golden_scene(name), flags=f, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=2) as r:
            r.render(0, FRAMES)
            shards += layers(r)  # a tile shard writes its own tiles and leaves the rest zero: adding zero is exact
    assert np.array_equal(shards, want), (name, flags)


@pytest.mark.gpu
def test_many_emitters_render_against_the_oracle(oracle_mod):
    """The `x % n` arms in a whole render: the bounds of the project's smoke run (T1), paths equal."""
    scene, _ = many_emitters()
    with api.Renderer(scene) as r:
        r.render(3, 8)
        gpu = r.download(0)
        st = r.stats().as_dict()
    o = oracle_mod.Oracle(scene)
    o.render(3, 8)
    ref = o.download(0)
    so = o.stats().as_dict()
    bad = (np.abs(gpu - ref) > 1e-2 * (1 + np.abs(ref))).any(axis=-1).mean()
    relmse = float(((gpu - ref) ** 2).sum() / (ref ** 2).sum())
    print(f"many-emitters against the oracle: bad pixels {bad:.3g}, relMSE {relmse:.3g}")
    assert bad <= 1e-3 and relmse <= 1e-4, (bad, relmse)
    assert st["paths"] == so["paths"]


@pytest.mark.gpu
def test_probe_refuses_what_has_no_table():
    with api.Renderer(scenes.veach_mis(64, 36)) as r:  # general BSDFs: the stream's position depends on the hit material
        with pytest.raises(api.ReneError) as e:
            r.frame_stream_probe(0, 4)
        assert e.value.code == -1
    with api.Renderer(scenes.cornell_box(32, 32)) as r:
        assert r.frame_stream_probe(0, 0).shape == (0, DEPTHS, 4)
        with pytest.raises(api.ReneError):
            r.frame_stream_probe(0, 65537)

"""GPU: the direct-light pass (rene_direct, rene_direct_samples; include/rene_hip.h), with flags 0 and FLAG_FORCE_BVH so that the item loop and the
BVH instantiations both run -- its sums against the oracle's depth-capped renders (Oracle.set_experiment(depth_cap=...)) under the tolerances
the project holds for a WHOLE render of the same scene; its records against the numpy restatement (tests/direct_reference.py) of its own samples,
bit for bit; the coin of the mixture against the oracle's generator; beauty - direct on one context; tile shards, frame cuts, adaptive contexts;
the refusals that need a device."""
import ctypes as C

import numpy as np
import pytest

import direct_reference as dref
import gbuffer_reference as gr
from gbuffer_reference import _assert_records_equal, _bits
from rene_amd import abi, api, scenes
from test_gpu_parity import t1_check

pytestmark = pytest.mark.gpu

FLAGS = (0, abi.FLAG_FORCE_BVH)
W, H = 48, 40  # Cornell: partial tiles on both axes
SUN = ((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))  # dragon/scene.pbrt:44, as tests/test_gpu_scenes.py:77-79 adds it


def _cornell():
    return scenes.cornell_box(W, H)


def _cornell_sun_no_emitter():
    s = scenes.cornell_box(W, H)
    s.instances[-1].area_light_index = 0  # switch the quad emitter off
    s.add_light_distant(*SUN)
    return s


def _cornell_sun():
    s = scenes.cornell_box(W, H)
    s.add_light_distant(*SUN)
    return s


def _zoo_without_its_light():
    s = scenes.material_zoo(96, 64)
    assert len(s.lights) == 1
    s.lights.clear()
    return s


# name -> (builder, frames of the tests)
SCENES = {"cornell": (_cornell, 8), "cornell-sun-no-emitter": (_cornell_sun_no_emitter, 8), "cornell+sun": (_cornell_sun, 8),
          "dragon": (lambda: scenes.dragon_class(80, 45, 48, 52), 4), "veach": (lambda: scenes.veach_mis(160, 90), 4),
          "zoo": (lambda: scenes.material_zoo(96, 64), 4), "zoo-no-light": (_zoo_without_its_light, 4)}
_scene, _capped, _device = {}, {}, {}


def scene(name):
    if name not in _scene:
        _scene[name] = SCENES[name][0]()
    return _scene[name]


def capped(name, cap, oracle_mod):
    """The oracle's render of the scene's frames with at most `cap` iterations per path, (H, W, 3) sums; once per process."""
    if (name, cap) not in _capped:
        o = oracle_mod.Oracle(scene(name))
        o.set_experiment(depth_cap=cap)
        o.render(0, SCENES[name][1])
        _capped[name, cap] = o.download(0)
    return _capped[name, cap]


def device(name, flags):
    """A context on the scene under `flags`, its records and its samples over the scene's frames; once per process."""
    if (name, flags) not in _device:
        r = api.Renderer(scene(name), flags=flags)
        n = SCENES[name][1]
        _device[name, flags] = {"r": r, "rec": r.direct(0, n), "samples": r.direct_samples(0, n)}
    return _device[name, flags]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for d in _device.values():
        d["r"].close()
    _device.clear()


def _against(got, ref, what, frac=1e-3, relmse=1e-4):
    """tests/test_gpu_scenes.py's _compare on one layer: non-finite pixels masked, then the T1 check with the named test's tolerances."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    fin = np.isfinite(got).all(axis=2) & np.isfinite(ref).all(axis=2)
    g, o = np.where(fin[..., None], got, 0), np.where(fin[..., None], ref, 0)
    diff = np.abs(g - o)
    print(what, "pixels off:", int((diff > 1e-2 * (1 + np.abs(o))).any(axis=-1).sum()), "of", fin.size, "allowed share", frac, "relMSE",
          float(((g - o) ** 2).sum() / max(1e-30, (o ** 2).sum())), "allowed", relmse, "non-finite", int((~fin).sum()))
    assert fin.mean() > 0.99, what
    t1_check(g, o, frac=frac, relmse=relmse)


def _first(rec):
    return rec["seen"] + rec["distant"]


def _basic(name, flags):
    d = device(name, flags)
    rec, n = d["rec"], SCENES[name][1]
    assert rec.shape == d["samples"].shape[1:] and (rec["n"] == n).all() and not rec["reserved"].any() and (rec["hits"] <= n).all()
    assert (d["samples"]["state"] <= dref.ENDED_ZERO).all() and (d["samples"]["second"] <= abi.DIRECT_SECOND_EMITTER).all()
    return d, rec


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_cornell_against_the_capped_renders(flags, oracle_mod):
    """seen + distant is the depth_cap = 1 render, direct_sum the depth_cap = 2 render (t1_check's defaults, tests/test_gpu_parity.py:26);
    distant == 0 exactly; hits is the geometry pass's of the same frames."""
    d, rec = _basic("cornell", flags)
    _against(_first(rec), capped("cornell", 1, oracle_mod), ("cornell", flags, "cap 1"))
    _against(api.direct_sum(rec), capped("cornell", 2, oracle_mod), ("cornell", flags, "cap 2"))
    assert not _bits(rec["distant"]).any()
    assert np.array_equal(rec["hits"], d["r"].gbuffer(0, 8)["hits"])
    s = d["samples"]
    assert ((s["state"] == dref.LIGHT) | (s["state"] == dref.BSDF)).mean() > 0.3 and rec["sampled"].sum() > 0 and rec["seen"].sum() > 0


@pytest.mark.parametrize("flags", FLAGS)
def test_cornell_under_a_distant_light_without_its_emitter(flags, oracle_mod):
    """seen + distant against cap 1 (test_cornell_with_distant_light_and_no_emitter's frac = 1e-3, relmse = 1e-4); no mixture anywhere."""
    d, rec = _basic("cornell-sun-no-emitter", flags)
    _against(_first(rec), capped("cornell-sun-no-emitter", 1, oracle_mod), ("cornell-sun-no-emitter", flags, "cap 1"), frac=1e-3, relmse=1e-4)
    s = d["samples"]
    assert rec["distant"].sum() > 0 and not rec["seen"].any() and not np.isin(s["state"], (dref.LIGHT, dref.BSDF)).any()


@pytest.mark.parametrize("flags", FLAGS)
def test_a_distant_light_changes_neither_seen_nor_sampled(flags, oracle_mod):
    """Cornell plus the light, emitter on: the light loop touches neither the throughput nor a generator, so seen and sampled are bit for bit
    those of the plain Cornell run; seen + distant against cap 1 (t1_check's defaults)."""
    d, rec = _basic("cornell+sun", flags)
    plain = device("cornell", flags)
    for k in ("seen", "sampled", "hits"):
        assert np.array_equal(_bits(rec[k]), _bits(plain["rec"][k])), k
    for k in ("seen", "sampled", "state", "second", "wi", "pdf"):
        assert np.array_equal(_bits(d["samples"][k]), _bits(plain["samples"][k])), k
    assert rec["distant"].sum() > 0
    _against(_first(rec), capped("cornell+sun", 1, oracle_mod), ("cornell+sun", flags, "cap 1"))


@pytest.mark.parametrize("flags", FLAGS)
def test_dragon_class_against_cap_one_and_plain_on_every_hit(flags, oracle_mod):
    """seen + distant against cap 1 (test_dragon_class_bvh_path's frac = 2e-3, relmse = 1e-4); no emitter: every hit sample is PLAIN."""
    d, rec = _basic("dragon", flags)
    _against(_first(rec), capped("dragon", 1, oracle_mod), ("dragon", flags, "cap 1"), frac=2e-3, relmse=1e-4)
    s = d["samples"]
    assert np.isin(s["state"], (dref.MISS, dref.PLAIN)).all() and (s["state"] == dref.PLAIN).mean() > 0.3
    assert np.array_equal(s["state"] != dref.MISS, d["r"].primary_hits(0, 4)["t"] >= 0)
    assert not rec["seen"].any() and not rec["sampled"].any()  # no emitter, a black background


@pytest.mark.parametrize("flags", FLAGS)
def test_veach_mis_against_cap_two(flags, oracle_mod):
    """direct_sum against cap 2 under test_veach_mis_metal_and_sphere_emitters' frac = 0.12, relmse = 1e-4 (the reason is given there: the cone
    pdf of the small sphere emitter cancels in fp32)."""
    d, rec = _basic("veach", flags)
    _against(api.direct_sum(rec), capped("veach", 2, oracle_mod), ("veach", flags, "cap 2"), frac=0.12, relmse=1e-4)
    _against(_first(rec), capped("veach", 1, oracle_mod), ("veach", flags, "cap 1"), frac=0.12, relmse=1e-4)
    s = d["samples"]  # (rene's Microfacet lobe counts as diffuse, bxdf.rs:357: Metal takes the mixture too)
    assert not _bits(rec["distant"]).any() and (s["state"] == dref.BSDF).any() and (s["state"] == dref.LIGHT).any() and rec["sampled"].sum() > 0


@pytest.mark.parametrize("flags", FLAGS)
def test_material_zoo_against_the_capped_renders(flags, oracle_mod):
    """seen + distant against cap 1; sampled against cap 2 - cap 1 of the zoo WITHOUT its distant light (the light loop touches neither the
    throughput nor a generator, and cap 2 of the zoo itself would hold iteration 1's light loop); test_material_zoo_every_kind's frac = 1e-2,
    relmse = 2e-3."""
    d, rec = _basic("zoo", flags)
    _against(_first(rec), capped("zoo", 1, oracle_mod), ("zoo", flags, "cap 1"), frac=1e-2, relmse=2e-3)
    ref = capped("zoo-no-light", 2, oracle_mod) - capped("zoo-no-light", 1, oracle_mod)
    _against(rec["sampled"], ref, ("zoo", flags, "cap 2 - cap 1"), frac=1e-2, relmse=2e-3)
    s = d["samples"]
    assert rec["distant"].sum() > 0 and (s["second"] == abi.DIRECT_SECOND_MISS).any() and (s["second"] == abi.DIRECT_SECOND_EMITTER).any()
    for state in (dref.MISS, dref.LIGHT, dref.BSDF, dref.PLAIN):
        assert (s["state"] == state).any(), state


# ---- the aggregate -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_records_are_the_restatement_of_the_own_samples(name, flags):
    d, rec = _basic(name, flags)
    _assert_records_equal(rec, dref.aggregate(d["samples"]), (name, flags))
    n = SCENES[name][1]
    _assert_records_equal(d["r"].direct(0, n - 1), dref.aggregate(d["samples"][:n - 1]), (name, flags, n - 1))
    s = d["samples"]
    miss = s[s["state"] == dref.MISS]
    assert not miss["distant"].any() and not miss["sampled"].any() and not miss["wi"].any() and not miss["pdf"].any() and not miss["second"].any()
    ended = s[np.isin(s["state"], (dref.ENDED_PDF, dref.ENDED_ZERO))]
    assert not ended["sampled"].any() and not ended["second"].any()
    assert not s["reserved"].any() and not s["sampled"][s["second"] == abi.DIRECT_SECOND_SURFACE].any()


# ---- the coin ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_the_coin_is_one_per_frame_and_the_light_samples_meet_in_one_point(flags, oracle_mod):
    """Per frame every LIGHT or BSDF sample has the state oracle.pcg_f32(seed_f, 1)[0] > 0.5 says; within a frame the lines position + t wi of all
    LIGHT samples meet in one point of the emitter quad (y = 1.98, x in -0.24 .. 0.23, z in -0.22 .. 0.16) to 1e-4: the least-squares point of the
    lines lies on the quad and every line passes it within 1e-4."""
    d, _ = _basic("cornell", flags)
    s, r = d["samples"], d["r"]
    seeds = api.frame_seeds(abi.DEFAULT_SEED, 0, 8)
    hits = r.primary_hits(0, 8)
    origin = gr.camera_origin(scene("cornell")).astype(np.float64)
    pos = origin + hits["t"].astype(np.float64)[..., None] * hits["d"].astype(np.float64)
    sides = set()
    for f, seed in enumerate(seeds):
        light = bool(oracle_mod.pcg_f32(int(seed), 1)[0] > 0.5)
        sides.add(light)
        mixed = np.isin(s["state"][f], (dref.LIGHT, dref.BSDF))
        assert mixed.mean() > 0.2 and (s["state"][f][mixed] == (dref.LIGHT if light else dref.BSDF)).all(), (f, light)
        if not light:
            continue
        p, w = pos[f][mixed], s["wi"][f][mixed].astype(np.float64)
        assert np.abs(np.linalg.norm(w, axis=-1) - 1).max() <= 1e-5
        # the point closest to all lines: sum (I - w w^T) q = sum (I - w w^T) p
        proj = np.eye(3)[None] - w[:, :, None] * w[:, None, :]
        q = np.linalg.solve(proj.sum(0), (proj @ p[:, :, None]).sum(0)[:, 0])
        dist = np.linalg.norm((proj @ (q - p)[:, :, None])[:, :, 0], axis=-1)
        print("frame", f, "the light samples' point", q, "largest distance of a line", dist.max(), "lines", len(p))
        assert abs(q[1] - 1.98) <= 1e-4 and -0.24 - 1e-4 <= q[0] <= 0.23 + 1e-4 and -0.22 - 1e-4 <= q[2] <= 0.16 + 1e-4, q
        assert dist.max() <= 1e-4, (f, dist.max())
    assert sides == {True, False}  # both sides of the coin occur among frames 0 .. 7


# ---- the same samples -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_beauty_minus_direct_is_the_indirect_light_of_the_same_samples(flags):
    """One context that rendered frames 0 .. 15, and the pass over frames 0 .. 15: beauty_sum - direct_sum >= -1e-2 (1 + beauty_sum) on all but
    0.1 % of the pixels (the T1 tier's per-pixel bound and share, for the rare forked decision), its image mean is positive, and the pass leaves
    download(0 .. 2) and rene_get_stats bit-identical."""
    with api.Renderer(scene("cornell"), flags=flags | abi.FLAG_COUNTERS) as r:
        r.render(0, 16)
        before = [r.download(l) for l in range(3)]
        st_before = bytes(r.stats())
        rec = r.direct(0, 16)
        r.direct_samples(3, 2)
        after = [r.download(l) for l in range(3)]
        st_after = bytes(r.stats())
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert st_before == st_after
    beauty, direct = before[0][..., :3], api.direct_sum(rec)
    low = (beauty - direct < -1e-2 * (1 + beauty)).any(axis=-1)
    print("pixels below the bound:", int(low.sum()), "of", low.size, "smallest difference", float((beauty - direct).min()))
    assert low.mean() <= 1e-3
    indirect = api.indirect_mean(before[0], rec)
    assert indirect.mean() > 0 and np.array_equal(indirect, (beauty - direct) / np.float32(16))
    assert direct.mean() > 0.2 * beauty.mean()  # (and the direct light is a good part of the Cornell box's)


# ---- shards and cuts -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_two_tile_shards_fill_one_tensor_and_merge(flags):
    import torch
    s = scenes.cornell_box(100, 70)  # 4 x 3 tiles
    with api.Renderer(s, flags=flags) as r:
        whole = r.direct(0, 8)
    assert (whole["n"] == 8).all()
    t = torch.full((70, 100, 48), 0xAB, dtype=torch.uint8, device="cuda")
    parts, acc = [], np.zeros(70 * 100 * 48, np.uint8)
    for rank in range(2):
        with api.Renderer(s, flags=flags, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=2) as r:
            parts.append(r.direct(0, 8))
            ptr, n = r.direct_buffer()
            assert ptr and n == 70 * 100 * 48 == api.direct_bytes(100, 70)
            smp = r.direct_samples(0, 2)
            assert r.direct_into(t, 0, 8) is t  # (all of it is written: zeros, then this shard's tiles)
            r.sync()
            got = t.cpu().numpy().reshape(-1)
        own = gr.owned_mask(100, 70, rank, 2)
        assert got.tobytes() == parts[-1].tobytes()
        assert parts[-1][~own].tobytes() == bytes(48 * int((~own).sum())) and (parts[-1]["n"][own] == 8).all()
        assert smp[:, ~own].tobytes() == bytes(64 * 2 * int((~own).sum()))
        acc |= got  # the shards' tiles are disjoint and the rest of either is zero: one tensor filled by both
    assert acc.tobytes() == whole.tobytes()
    assert api.direct_merge(parts).tobytes() == whole.tobytes()
    t32 = torch.full((70, 100, 12), -1, dtype=torch.int32, device="cuda")
    with api.Renderer(s, flags=flags) as r:
        assert r.direct_into(t32, 0, 8) is t32
        r.sync()
    assert t32.cpu().numpy().tobytes() == whole.tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_two_ranges_of_frames_add_up_to_the_whole(flags):
    """Frames 0 .. 7 and then 8 .. 15, added by the reference's rule in numpy, equal 0 .. 15: hits exactly, the sums to fp32 rounding (16 adds of
    non-negative terms in another association: 16 2^-24 relative, and the same again for slack)."""
    r = device("cornell", flags)["r"]
    a, b, whole = r.direct(0, 8), r.direct(8, 8), r.direct(0, 16)
    assert np.array_equal(a["hits"] + b["hits"], whole["hits"]) and (whole["n"] == 16).all()
    _assert_records_equal(a, device("cornell", flags)["rec"], "the result does not depend on what ran before")
    for k in ("seen", "distant", "sampled"):
        got = a[k] + b[k]
        assert np.abs(got - whole[k]).max() <= 32 * 2.0 ** -24 * np.abs(whole[k]).max(), k
        np.testing.assert_allclose(got, whole[k], rtol=32 * 2.0 ** -24, atol=0)


def test_an_adaptive_context_and_a_reset_give_the_plain_records():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r:
        even = r.direct(0, 8)
    with api.Renderer(s) as r:
        r.render(0, 8)
        active = np.indices((3, 4)).sum(0) % 2  # half of the tiles go on
        r.set_active_tiles(active)
        r.render(8, 8)
        assert r.direct(0, 8).tobytes() == even.tobytes()
        assert sorted(set(r.tile_frames().reshape(-1).tolist())) == [8, 16]  # (the mask was in force, and still is)
    with api.Renderer(s) as r:
        r.direct(0, 8)
        r.reset()
        assert api._download_result(r, api.lib().rene_download_direct, (70, 100), abi.DIRECT_DTYPE).tobytes() == even.tobytes()  # (a reset does not invalidate it)


# ---- refusals that need a device -----------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_device():
    import torch
    r = device("cornell", 0)["r"]
    p = api.direct_params_default()
    need = api.direct_bytes(W, H)
    t = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    host = np.zeros(need + 16, np.uint8)
    cases = ((host.ctypes.data, need), (t.data_ptr(), need - 1), (t.data_ptr() + 4, need))  # a host pointer; short; misaligned
    for dst, size in cases:
        with pytest.raises(api.ReneError) as e:
            api._check(api.lib().rene_direct(r._h, C.byref(p), C.c_void_p(dst), size))
        assert e.value.code == -1, (dst, size)
    assert not t.cpu().numpy().any()  # nothing was launched
    with pytest.raises(ValueError):
        r.direct_into(torch.zeros(need - 48, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        r.direct_into(torch.zeros(need // 4, dtype=torch.float32, device="cuda"))
    one = np.zeros(1, abi.DIRECT_SAMPLE_DTYPE)  # more than 2^22 records: refused before the destination is looked at
    p.n_frames = 65536
    assert api.lib().rene_direct_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"2^22" in api.lib().rene_last_error()
    p.n_frames = 2
    assert api.lib().rene_direct_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"smaller" in api.lib().rene_last_error()
    with api.Renderer(scenes.cornell_fog(32, 32)) as fog:
        for call in (lambda: fog.direct(0, 2), lambda: fog.direct_samples(0, 1)):
            with pytest.raises(api.ReneError) as e:
                call()
            assert e.value.code == -4 and "volpath" in str(e.value)  # RENE_ERR_UNSUPPORTED, and the message says why

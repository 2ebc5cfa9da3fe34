"""GPU: the light-group pass (rene_lights, rene_lights_samples; include/rene_hip.h), with flags 0 and FLAG_FORCE_BVH so that the item loop and the BVH
instantiations both run, on tests/lights_scenes.py's scenes -- the Cornell box at 72 x 40 with two lamps and a sun (Matte form), the material zoo
(general form: a textured background, a distant light, a triangle and a sphere emitter) and deep_paths.  Its records against the numpy
restatement (tests/lights_reference.py) of its own samples, bit for bit; each group against the SAME pass on the scene with every other source
black, bit for bit (tests/test_lights_reference.py shows on the CPU that blacking leaves the paths alone); the groups' total against the bounce
pass of the same context; each group against the oracle's render of the blacked scene; the caller's grouping; the re-mix; tile shards, frame
cuts, adaptive contexts; the refusals that need a device."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_reference as gr
import lights_reference as lref
import lights_scenes
from gbuffer_reference import _assert_records_equal, _bits
from rene_amd import abi, api, scenes
from test_gpu_direct import _against

pytestmark = pytest.mark.gpu

FLAGS = (0, abi.FLAG_FORCE_BVH)
# name -> (builder, frames of the tests, share of pixels off and relMSE the project allows a whole render of such a scene: tests/test_gpu_direct.py's
# "cornell+sun" and "zoo" rows)
SCENES = {"cornell": (lights_scenes.cornell, 8, 1e-3, 1e-4), "zoo": (lights_scenes.zoo, 4, 1e-2, 2e-3), "deep": (lights_scenes.deep, 8, None, None)}
FORKED = 1e-3  # the share of pixels tests/test_gpu_bounces.py allows off the render kernels' image, for paths that fork on a rounded decision
_scene, _device, _black = {}, {}, {}


def scene(name):
    if name not in _scene:
        _scene[name] = SCENES[name][0]()
    return _scene[name]


def frames(name):
    return SCENES[name][1]


def device(name, flags):
    """A context on the scene under `flags`, its records and samples under the library's grouping over the scene's frames; once per process."""
    if (name, flags) not in _device:
        r = api.Renderer(scene(name), flags=flags)
        n = frames(name)
        groups, used = r.light_groups()
        _device[name, flags] = {"r": r, "rec": r.lights(0, n), "samples": r.lights_samples(0, n), "groups": groups, "used": used}
    return _device[name, flags]


def blacked(name, flags, g):
    """The pass's records on the scene with every source outside group g black; once per process."""
    if (name, flags, g) not in _black:
        with api.Renderer(lights_scenes.only(SCENES[name][0], g), flags=flags) as r:
            _black[name, flags, g] = r.lights(0, frames(name))
    return _black[name, flags, g]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for d in _device.values():
        d["r"].close()
    _device.clear()


def _basic(name, flags):
    d = device(name, flags)
    rec, s, n = d["rec"], d["samples"], frames(name)
    (inst, dist, bg), used = lights_scenes.default_groups(scene(name))
    assert d["used"] == used and d["groups"][2] == bg and np.array_equal(d["groups"][0], inst) and np.array_equal(d["groups"][1], dist)
    assert rec.shape == s.shape[1:] == (scene(name).film.yresolution, scene(name).film.xresolution)
    assert (rec["n"] == n).all() and (s["n"] == 1).all() and not rec["reserved"].any() and (s["lit"] <= 1).all()
    assert (s["end"] <= abi.BOUNCES_END_CAP).all() and (s["length"] >= 1).all() and (s["length"] <= 50).all()
    assert np.array_equal(s["lit"] != 0, s["group"]["adds"].sum(axis=-1) != 0)  # lit: any add that was not black
    if used < 8:
        assert not _bits(rec["group"][:, :, used:]).any() and not _bits(s["group"][:, :, :, used:]).any()  # nothing maps beyond the groups in use
    return d, rec


def _bound(a, b, n_frames, lights_len):
    """Two fp32 folds of the same non-negative terms in another order: at most M = n_frames x 50 x (2 + lights_len) terms, each with one rounding of
    its product, and two fold orders -- per pixel and channel |a - b| <= 4 M 2^-24 max(a, b).  Returns the pixels off it, non-finite ones masked."""
    M = n_frames * 50 * (2 + lights_len)
    fin = np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1)
    a, b = np.where(fin[..., None], a, 0).astype(np.float64), np.where(fin[..., None], b, 0).astype(np.float64)
    return (np.abs(a - b) > 4 * M * 2.0 ** -24 * np.maximum(a, b)).any(axis=-1), fin


# ---- the aggregate -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(SCENES))
def test_records_are_the_restatement_of_the_own_samples(name, flags):
    d, rec = _basic(name, flags)
    s = d["samples"]
    _assert_records_equal(rec, lref.pixel_records(s), (name, flags))
    assert np.array_equal(rec["group"]["adds"], s["group"]["adds"].sum(axis=0, dtype=np.uint32)) and np.array_equal(rec["lit"], s["lit"].sum(axis=0, dtype=np.uint32))
    assert not _bits(s["group"]["sum"])[s["group"]["adds"] == 0].any()  # + 0 where the sample has nothing that is not black
    assert not np.signbit(rec["group"]["sum"]).any() and not np.signbit(s["group"]["sum"]).any()  # (no sum is ever - 0)
    assert BITS_EQUAL(api.lights_sum(rec), lref.total(rec)) and rec["lit"].sum() > 0
    print(name, flags, "adds per group:", rec["group"]["adds"].sum(axis=(0, 1)).tolist(), "lit samples:", int(rec["lit"].sum()), "of", rec["n"].sum())


def BITS_EQUAL(a, b):
    return _bits(np.asarray(a, np.float32)).tobytes() == _bits(np.asarray(b, np.float32)).tobytes()


# ---- a group is the job with the other sources black ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_a_group_is_the_pass_on_the_scene_with_the_other_sources_black(name, flags):
    d, rec = _basic(name, flags)
    for g in range(d["used"]):
        black = blacked(name, flags, g)
        assert black["group"][:, :, g].tobytes() == rec["group"][:, :, g].tobytes(), (name, flags, g)  # sums and adds
        others = [k for k in range(8) if k != g]
        assert not _bits(black["group"][:, :, others]).any(), (name, flags, g)  # every other group: all-zero words
        assert np.array_equal(black["lit"] != 0, black["group"]["adds"][:, :, g] != 0) and (black["n"] == frames(name)).all()


# ---- the groups add up to the bounce pass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_groups_add_up_to_the_bounce_pass(name, flags):
    d, rec = _basic(name, flags)
    r, n = d["r"], frames(name)
    bounces, bs = r.bounces(0, n), r.bounces_samples(0, n)
    off, fin = _bound(api.lights_sum(rec), api.bounces_sum(bounces), n, len(scene(name).lights))
    differ = (d["samples"]["length"] != bs["length"]) | (d["samples"]["end"] != bs["end"])
    print(name, flags, "pixels off the bound:", int(off.sum()), "of", off.size, "non-finite:", int((~fin).sum()), "samples whose length or end differ:", int(differ.sum()))
    assert off.mean() <= FORKED and differ.mean() <= FORKED and fin.mean() > 0.99


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_every_group_against_the_oracles_render_of_the_blacked_scene(name, flags, oracle_mod):
    d, rec = _basic(name, flags)
    _, n, frac, relmse = SCENES[name]
    for g in range(d["used"]):
        ref = lref.oracle_only(name, SCENES[name][0], g, n, oracle_mod)["image"]
        got = api.lights_group_sum(rec, g)
        if not np.nan_to_num(ref).any():
            assert not _bits(rec["group"][:, :, g]).any(), (name, flags, g)  # a group the oracle leaves empty is empty here
            continue
        assert np.nan_to_num(got).any(), (name, flags, g)
        _against(got, ref, (name, flags, "group", g), frac=frac, relmse=relmse)
        mean = api.lights_group_mean(rec, g)
        assert BITS_EQUAL(mean, lref.group_mean(rec, g))
        _against(mean, ref / np.float32(n), (name, flags, "group", g, "per sample"), frac=frac, relmse=relmse)


# ---- grouping is the caller's ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_the_grouping_is_the_callers(name, flags):
    d, rec = _basic(name, flags)
    r, n, s = d["r"], frames(name), scene(name)
    inst, dist, bg = d["groups"]
    one = r.lights(0, n, groups=(np.full_like(inst, 3), np.full_like(dist, 3), 3))
    assert not _bits(one["group"][:, :, [0, 1, 2, 4, 5, 6, 7]]).any()  # only group 3 is filled
    assert np.array_equal(one["group"]["adds"][:, :, 3], rec["group"]["adds"].sum(axis=-1, dtype=np.uint32)) and np.array_equal(one["lit"], rec["lit"])
    off, fin = _bound(api.lights_sum(one), api.lights_sum(rec), n, len(s.lights))
    print(name, flags, "one group against the default grouping's total, pixels off the bound:", int(off.sum()), "non-finite:", int((~fin).sum()))
    assert off.mean() <= FORKED
    a, b = lights_scenes.emitting(s)[:2]
    swapped = inst.copy()
    swapped[a], swapped[b] = inst[b], inst[a]
    swap = r.lights(0, n, groups=(swapped, dist, bg))
    ga, gb = int(inst[a]), int(inst[b])
    assert swap["group"][:, :, ga].tobytes() == rec["group"][:, :, gb].tobytes() and swap["group"][:, :, gb].tobytes() == rec["group"][:, :, ga].tobytes()
    rest = [k for k in range(8) if k not in (ga, gb)]
    assert swap["group"][:, :, rest].tobytes() == rec["group"][:, :, rest].tobytes() and rec["group"]["adds"][:, :, ga].sum() > 0 < rec["group"]["adds"][:, :, gb].sum()
    _assert_records_equal(r.lights(0, n, groups=d["groups"]), rec, "the library's grouping, handed in")
    assert r.lights_samples(0, n, groups=d["groups"]).tobytes() == d["samples"].tobytes()


def test_more_sources_than_groups_share_the_last_one():
    s = lights_scenes.many_sources()
    with api.Renderer(s) as r:
        (inst, dist, bg), used = r.light_groups()
        want, want_used = lights_scenes.default_groups(s)
        assert used == want_used == 8 and bg == 0 and dist.tolist() == [1, 2, 3] and np.array_equal(inst, want[0])
        assert inst[lights_scenes.emitting(s)].tolist() == [4, 5, 6, 7, 7, 7]
        rec = r.lights(0, 4)
        each = inst.copy()
        each[lights_scenes.emitting(s)[3:]] = [7, 0, 0]  # the overflow's first lamp alone in group 7, the two others with the (black) background
        split = r.lights(0, 4, groups=(each, dist, bg))
    assert (rec["group"]["adds"][:, :, 1:].sum(axis=(0, 1)) > 0).all() and not _bits(rec["group"][:, :, 0]).any()
    assert np.array_equal(split["group"]["adds"][:, :, 7] + split["group"]["adds"][:, :, 0], rec["group"]["adds"][:, :, 7])
    assert split["group"][:, :, 1:7].tobytes() == rec["group"][:, :, 1:7].tobytes()


# ---- the re-mix --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_the_mix_with_one_weight_doubled_is_the_scene_with_that_source_doubled(name, flags):
    d, rec = _basic(name, flags)
    n = frames(name)
    ones = np.ones(8, np.float32)
    unit = api.lights_mix(rec, ones)
    assert BITS_EQUAL(unit, lref.mix(rec, ones)) and BITS_EQUAL(unit, api.lights_sum(rec) / np.float32(n))
    g = d["used"] - 1  # the last emitting instance
    w = ones.copy()
    w[g] = 2
    with api.Renderer(lights_scenes.scaled(SCENES[name][0], g, 2), flags=flags) as r:
        twice = r.lights(0, n)
    mixed = api.lights_mix(rec, w)
    assert BITS_EQUAL(mixed, lref.mix(rec, w))
    off, fin = _bound(mixed * np.float32(n), api.lights_sum(twice), n, len(scene(name).lights))
    print(name, flags, "the mix with group", g, "doubled against the doubled scene, pixels off the bound:", int(off.sum()), "non-finite:", int((~fin).sum()))
    assert off.mean() <= FORKED and fin.mean() > 0.99
    assert twice["group"][:, :, :g].tobytes() == rec["group"][:, :, :g].tobytes()  # (the other groups do not move; 2 x is exact, so neither do the paths)
    assert np.array_equal(twice["group"]["sum"][:, :, g], np.float32(2) * rec["group"]["sum"][:, :, g], equal_nan=True)
    assert np.array_equal(twice["group"]["adds"], rec["group"]["adds"])


# ---- shards and cuts -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_three_tile_shards_merge_and_two_fill_one_tensor(flags):
    import torch
    s, n = scene("cornell"), frames("cornell")  # 72 x 40: 3 x 2 tiles
    _, whole = _basic("cornell", flags)
    parts = []
    for rank in range(3):
        with api.Renderer(s, flags=flags, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            parts.append(r.lights(0, n))
            ptr, nbytes = r.lights_buffer()
            assert ptr and nbytes == 40 * 72 * 144 == api.lights_bytes(72, 40)
            smp = r.lights_samples(0, 1)
        own = gr.owned_mask(72, 40, rank, 3)
        assert parts[-1][~own].tobytes() == bytes(144 * int((~own).sum())) and (parts[-1]["n"][own] == n).all()
        assert smp[:, ~own].tobytes() == bytes(144 * int((~own).sum())) and (smp["n"][0][own] == 1).all()
    _assert_records_equal(api.lights_merge(parts), whole, ("three shards", flags))
    t = torch.full((40, 72, 144), 0xAB, dtype=torch.uint8, device="cuda")
    acc = np.zeros(40 * 72 * 144, np.uint8)
    for rank in range(2):
        with api.Renderer(s, flags=flags, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=2) as r:
            assert r.lights_into(t, 0, n) is t  # (all of it is written: zeros, then this shard's tiles)
            r.sync()
            acc |= t.cpu().numpy().reshape(-1)  # the shards' tiles are disjoint and the rest of either is zero: one tensor filled by both
    assert acc.tobytes() == whole.tobytes()
    t32 = torch.full((40, 72, 36), -1, dtype=torch.int32, device="cuda")
    with api.Renderer(s, flags=flags) as r:
        assert r.lights_into(t32, 0, n) is t32
        r.sync()
    assert t32.cpu().numpy().tobytes() == whole.tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_two_ranges_of_frames_are_the_whole_ranges_rows(flags):
    d, first = _basic("cornell", flags)
    r = d["r"]
    whole_s, head_s, tail_s = r.lights_samples(0, 8), r.lights_samples(0, 4), r.lights_samples(4, 4)
    assert head_s.tobytes() == whole_s[:4].tobytes() and tail_s.tobytes() == whole_s[4:].tobytes() and d["samples"].tobytes() == whole_s.tobytes()
    a, b = r.lights(0, 4), r.lights(4, 4)
    _assert_records_equal(r.lights(0, 8), first, "the result does not depend on what ran before")
    _assert_records_equal(a, lref.pixel_records(head_s), "frames 0 .. 3")
    _assert_records_equal(b, lref.pixel_records(tail_s), "frames 4 .. 7")
    for k in ("n", "lit"):
        assert np.array_equal(a[k] + b[k], first[k]), k
    assert np.array_equal(a["group"]["adds"] + b["group"]["adds"], first["group"]["adds"])


# ---- contexts -------------------------------------------------------------------------------------------------------------------------------------------
def test_an_adaptive_context_a_reset_and_a_rendered_contexts_layers():
    s = lights_scenes.cornell(100, 70)
    with api.Renderer(s) as r:
        even = r.lights(0, 8)
    with api.Renderer(s) as r:
        r.render(0, 8)
        active = np.indices((3, 4)).sum(0) % 2  # half of the tiles go on
        r.set_active_tiles(active)
        r.render(8, 8)
        before = [r.download(l) for l in range(3)]
        st_before = bytes(r.stats())
        assert r.lights(0, 8).tobytes() == even.tobytes()
        r.lights_samples(3, 2)
        after = [r.download(l) for l in range(3)]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)) and st_before == bytes(r.stats())  # the accumulation layers: untouched
        assert sorted(set(r.tile_frames().reshape(-1).tolist())) == [8, 16]  # (the mask was in force, and still is)
    with api.Renderer(s) as r:
        r.lights(0, 8)
        r.reset()
        assert api._download_result(r, api.lib().rene_download_lights, (70, 100), abi.LIGHTS_DTYPE).tobytes() == even.tobytes()  # (a reset does not invalidate it)


def test_refusals_that_need_a_device():
    import torch
    d = device("cornell", 0)
    r = d["r"]
    W, H = r.xres, r.yres
    inst, dist, bg = d["groups"]
    p = api.lights_params_default()
    need = api.lights_bytes(W, H)
    t = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    host = np.zeros(need + 16, np.uint8)
    cases = ((host.ctypes.data, need), (t.data_ptr(), need - 1), (t.data_ptr() + 4, need))  # a host pointer; short; misaligned
    for dst, size in cases:
        with pytest.raises(api.ReneError) as e:
            api._check(api.lib().rene_lights(r._h, C.byref(p), C.c_void_p(dst), size))
        assert e.value.code == -1, (dst, size)
    assert not t.cpu().numpy().any()  # nothing was launched
    with pytest.raises(ValueError):
        r.lights_into(torch.zeros(need - 144, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        r.lights_into(torch.zeros(need // 4, dtype=torch.float32, device="cuda"))
    with pytest.raises((TypeError, ValueError)):
        r.lights_into(torch.zeros(need, dtype=torch.uint8))  # host memory
    # a count that is not the scene's; an entry of 8
    for groups, word in (((inst[:-1], dist, bg), "n_instances"), ((inst, np.zeros(2, np.uint8), bg), "n_distant"), ((inst, dist[:0], bg), "n_distant")):
        for call in (lambda: r.lights(0, 2, groups=groups), lambda: r.lights_samples(0, 1, groups=groups)):
            with pytest.raises(api.ReneError) as e:
                call()
            assert e.value.code == -1 and word in str(e.value), word
    eight = inst.copy()
    eight[-1] = 8
    for groups in ((eight, dist, bg), (inst, np.full_like(dist, 8), bg), (inst, dist, 8)):
        with pytest.raises(api.ReneError) as e:
            r.lights(0, 2, groups=groups)
        assert e.value.code == -1 and "below 8" in str(e.value)
    with pytest.raises(api.ReneError) as e:
        api._check(api.lib().rene_lights_default_groups(r._h, None, 0, None, 0, None, None))
    assert e.value.code == -1 and "the scene's" in str(e.value)
    _assert_records_equal(r.lights(0, frames("cornell")), d["rec"], "the refused calls left the context as it was")
    one = np.zeros(1, abi.LIGHTS_SAMPLE_DTYPE)  # more than 2^20 records: refused before the destination is looked at
    p.n_frames = 65536
    assert api.lib().rene_lights_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"2^20" in api.lib().rene_last_error()
    p.n_frames = 2
    assert api.lib().rene_lights_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"smaller" in api.lib().rene_last_error()
    with api.Renderer(scenes.cornell_fog(32, 32)) as fog:
        for call in (lambda: fog.lights(0, 2), lambda: fog.lights_samples(0, 1)):
            with pytest.raises(api.ReneError) as e:
                call()
            assert e.value.code == -4 and "volpath" in str(e.value)  # RENE_ERR_UNSUPPORTED, and the message says why

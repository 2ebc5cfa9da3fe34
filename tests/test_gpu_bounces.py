"""GPU: the bounce pass (rene_bounces, rene_bounces_samples; include/rene_hip.h), with flags 0 and FLAG_FORCE_BVH so that the item loop and the BVH
instantiations both run -- its cumulative sums against the CPU oracle's decomposition by bounce under the tolerances the project holds for a
WHOLE render of the same scene (a cumulative sum IS a depth-capped render: tests/test_bounces_reference.py); its records against the numpy
restatement (tests/bounces_reference.py) of its own samples, bit for bit; its first two buckets against the direct-light pass, bit for bit where
that must hold; the cap; its total against the render kernels' image of the same seeds; tile shards, frame cuts, adaptive contexts; the refusals
that need a device."""
import ctypes as C

import numpy as np
import pytest

import bounces_reference as bref
import emit_fusion_scenes
import gbuffer_reference as gr
from gbuffer_reference import _assert_records_equal, _bits
from rene_amd import abi, api, scenes
from test_gpu_direct import SCENES as DIRECT_SCENES
from test_gpu_direct import _against
from test_gpu_direct import scene as direct_scene

pytestmark = pytest.mark.gpu

FLAGS = (0, abi.FLAG_FORCE_BVH)
# name -> (frames of the tests, share of pixels off and relMSE the project allows a whole render of the scene: tests/test_gpu_direct.py cites each)
TABLE = {"cornell": (8, 1e-3, 1e-4), "dragon": (4, 2e-3, 1e-4), "veach": (4, 0.12, 1e-4), "zoo": (4, 1e-2, 2e-3)}
DEEP_FRAMES = 8
# |sum of length_sum - the oracle's rays_closest| / rays_closest on deep_paths under caps 13 and 14: paths fork where an fp32 decision falls the
# other way on the device, so this is measured, not derived -- per form of the closest-hit query twice the larger of the two figures an MI355X
# gave.  The item loop: 31 031 against 32 142 (3.457e-2) and 31 156 against 32 285 (3.497e-2); the BVH: 31 951 (5.94e-3) and 32 076 (6.47e-3).
# The render kernels fork the same way: their rays_closest over these frames is the pass's length_sum to the ray
FORK_MARGIN = {0: 2 * 3.497e-2, abi.FLAG_FORCE_BVH: 2 * 6.474e-3}
_scene, _device = {}, {}


def scene(name):
    if name == "deep":
        if name not in _scene:
            _scene[name] = emit_fusion_scenes.deep_paths(32, 32)
        return _scene[name]
    return direct_scene(name)


def frames(name):
    return DEEP_FRAMES if name == "deep" else TABLE[name][0]


def device(name, flags):
    """A context on the scene under `flags`, its records and its samples over the scene's frames; once per process."""
    if (name, flags) not in _device:
        r = api.Renderer(scene(name), flags=flags)
        n = frames(name)
        _device[name, flags] = {"r": r, "rec": r.bounces(0, n), "samples": r.bounces_samples(0, n)}
    return _device[name, flags]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for d in _device.values():
        d["r"].close()
    _device.clear()


def _basic(name, flags):
    d = device(name, flags)
    rec, s, n = d["rec"], d["samples"], frames(name)
    assert rec.shape == s.shape[1:] and (rec["n"] == n).all() and (s["n"] == 1).all() and not s["reserved"].any()
    assert (s["end"] <= bref.CAP).all() and (s["length"] >= 1).all() and (s["length"] <= 50).all()
    assert np.array_equal(s["bucket"]["reached"].sum(axis=-1), s["length"])  # every iteration falls into one bucket
    assert (s["bucket"]["reached"][..., :9] <= 1).all() and (rec["bucket"]["reached"][..., 0] == n).all()
    assert (np.diff(s["bucket"]["reached"][..., :9].astype(np.int64), axis=-1) <= 0).all()  # a path that made iteration d made d - 1
    return d, rec


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(TABLE))
def test_cumulative_sums_against_the_oracles_decomposition(name, flags, oracle_mod):
    """bounces_sum(rec, upto=k) against the oracle's adds at iterations 0 .. k - 1 of the same frames, k = 1, 2, 3, 5, 10, under the scene's
    whole-render tolerance (t1_check, non-finite pixels masked); the buckets the oracle fills are the ones the pass fills."""
    _, rec = _basic(name, flags)
    n, frac, relmse = TABLE[name]
    assert n == DIRECT_SCENES[name][1]
    dec = bref.decomposition(name, scene(name), n, oracle_mod)
    for k in (1, 2, 3, 5, 10):
        _against(api.bounces_sum(rec, upto=k), bref.cumulative(dec, k), (name, flags, "iterations 0 ..", k - 1), frac=frac, relmse=relmse)
    mine = [d for d in range(10) if np.nan_to_num(rec["bucket"]["sum"][:, :, d]).any()]
    theirs = [d for d in range(10) if np.nan_to_num(dec["layers"][d]).any()]
    print(name, flags, "buckets filled:", mine, "the oracle's:", theirs, "mean path length:", float(api.bounces_mean_length(rec).mean()))
    assert set(mine) >= set(theirs[:4])  # (a deep bucket with a handful of paths may fork empty on either side)


# ---- the aggregate -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(TABLE) + ["deep"])
def test_records_are_the_restatement_of_the_own_samples(name, flags):
    d, rec = _basic(name, flags)
    _assert_records_equal(rec, bref.pixel_records(d["samples"]), (name, flags))
    assert np.array_equal(api.bounces_sum(rec), bref.sum_upto(rec)) and np.array_equal(api.bounces_reached(rec), rec["bucket"]["reached"])
    s = d["samples"]
    unreached = s["bucket"]["reached"] == 0
    assert not _bits(s["bucket"]["sum"])[unreached].any()  # + 0 where the sample has nothing
    assert not np.signbit(rec["bucket"]["sum"]).any()      # (no sum is ever - 0: what lets the kernel skip a bucket no lane of the wave reached)


# ---- the direct-light pass ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["cornell", "veach"])
def test_the_first_two_buckets_are_the_direct_pass_bit_for_bit(name, flags):
    """No distant light in either scene and a throughput of 1 x at iteration 0: bucket[0].sum is the direct pass's `seen` and bucket[1].sum its
    `sampled` as bit patterns; bucket[1].reached counts the direct samples that made a second query."""
    d, rec = _basic(name, flags)
    n = frames(name)
    direct, dsamples = d["r"].direct(0, n), d["r"].direct_samples(0, n)
    assert not _bits(direct["distant"]).any()
    assert np.array_equal(_bits(rec["bucket"]["sum"][:, :, 0]), _bits(direct["seen"]))
    assert np.array_equal(_bits(rec["bucket"]["sum"][:, :, 1]), _bits(direct["sampled"]))
    assert np.array_equal(rec["bucket"]["reached"][:, :, 1], (dsamples["second"] != abi.DIRECT_SECOND_NONE).sum(axis=0))
    assert (rec["bucket"]["reached"][:, :, 0] == n).all() and rec["bucket"]["sum"][:, :, 1].sum() > 0


# ---- the cap ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_the_cap_cuts_the_paths_and_nothing_before_it(flags, oracle_mod):
    d, whole = _basic("deep", flags)
    r = d["r"]
    ends = d["samples"]["end"]
    print("deep_paths, flags", flags, "uncapped: longest path", int(whole["length_max"].max()), "samples by end (MISS, PDF, ZERO, ROULETTE, CAP):",
          [int((ends == e).sum()) for e in range(5)])
    assert not whole["capped"].any() and not (ends == bref.CAP).any() and whole["length_max"].max() >= 14  # iteration 13 is reached: a cap of 13 cuts
    _assert_records_equal(r.bounces(0, DEEP_FRAMES, max_depth=50), whole, "max_depth 0 is 50")
    total = {}
    for D in (1, 2, 13, 14):
        rec, s = r.bounces(0, DEEP_FRAMES, max_depth=D), r.bounces_samples(0, DEEP_FRAMES, max_depth=D)
        _assert_records_equal(rec, bref.pixel_records(s), ("deep", flags, D))
        for b in range(min(D, 9)):
            assert rec["bucket"][:, :, b].tobytes() == whole["bucket"][:, :, b].tobytes(), (D, b)
        if D <= 9:
            assert not rec["bucket"][:, :, D:].tobytes().strip(b"\0"), D
        assert rec["length_max"].max() <= D and (s["length"] <= D).all()
        assert np.array_equal(rec["capped"], (s["end"] == bref.CAP).sum(axis=0)) and (s["length"][s["end"] == bref.CAP] == D).all()
        total[D] = int(rec["length_sum"].sum(dtype=np.uint64))
        if D == 13:
            assert rec["capped"].sum() > 0
    assert total[1] == 32 * 32 * DEEP_FRAMES and total[2] > total[1] and total[13] < total[14] <= int(whole["length_sum"].sum(dtype=np.uint64))
    for D in (13, 14):
        o = oracle_mod.Oracle(scene("deep"))
        o.set_experiment(depth_cap=D)
        o.render(0, DEEP_FRAMES)
        want = o.stats().as_dict()["rays_closest"]
        rel = abs(total[D] - want) / want
        print("deep_paths, flags", flags, "cap", D, "closest-hit queries:", total[D], "the oracle's:", want, "relative difference:", rel, "allowed:", FORK_MARGIN[flags])
        assert want == {13: 32142, 14: 32285}[D] and rel <= FORK_MARGIN[flags], (D, total[D], want)
    with pytest.raises(api.ReneError) as e:
        r.bounces(0, 2, max_depth=51)
    assert e.value.code == -1 and "max_depth" in str(e.value)


# ---- the render kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("cornell", 0), ("cornell", abi.FLAG_FORCE_BVH), ("dragon", 0)])
def test_the_total_is_the_render_kernels_image_of_the_same_seeds(name, flags):
    """One context that rendered frames 0 .. 15 (Cornell: the item loop and the while-while kernel; dragon-class: the traversal-restart kernel)
    and the pass over frames 0 .. 15: |bounces_sum - beauty_sum| <= 1e-2 (1 + beauty_sum) on all but 0.1 % of the pixels (the T1 tier's per-pixel
    bound and share, for the rare forked decision), and the pass leaves download(0 .. 2) and rene_get_stats bit-identical."""
    with api.Renderer(scene(name), flags=flags | abi.FLAG_COUNTERS) as r:
        r.render(0, 16)
        before = [r.download(l) for l in range(3)]
        st_before = bytes(r.stats())
        rec = r.bounces(0, 16)
        r.bounces_samples(3, 2)
        after = [r.download(l) for l in range(3)]
        st_after = bytes(r.stats())
        counted = r.stats().as_dict()["rays_closest"]
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert st_before == st_after
    print(name, flags, "the render kernels' closest-hit queries:", counted, "the pass's length_sum:", int(rec["length_sum"].sum(dtype=np.uint64)))
    beauty, total = before[0][..., :3], api.bounces_sum(rec)
    fin = np.isfinite(beauty).all(axis=-1) & np.isfinite(total).all(axis=-1)
    diff = np.abs(np.where(fin[..., None], total - beauty, 0))
    off = (diff > 1e-2 * (1 + np.where(fin[..., None], beauty, 0))).any(axis=-1) | ~fin
    print(name, flags, "pixels off:", int(off.sum()), "of", off.size, "non-finite:", int((~fin).sum()), "largest difference:", float(diff.max()),
          "largest relative to 1 + beauty:", float((diff / (1 + np.where(fin[..., None], beauty, 0))).max()))
    assert off.mean() <= 1e-3 and total.mean() > 0


# ---- shards and cuts -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_three_tile_shards_merge_and_two_fill_one_tensor(flags):
    import torch
    s, n = scene("dragon"), frames("dragon")  # 80 x 45: 3 x 2 tiles
    _, whole = _basic("dragon", flags)
    parts = []
    for rank in range(3):
        with api.Renderer(s, flags=flags, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            parts.append(r.bounces(0, n))
            ptr, nbytes = r.bounces_buffer()
            assert ptr and nbytes == 45 * 80 * 176 == api.bounces_bytes(80, 45)
            smp = r.bounces_samples(0, 1)
        own = gr.owned_mask(80, 45, rank, 3)
        assert parts[-1][~own].tobytes() == bytes(176 * int((~own).sum())) and (parts[-1]["n"][own] == n).all()
        assert smp[:, ~own].tobytes() == bytes(176 * int((~own).sum())) and (smp["n"][0][own] == 1).all()
    _assert_records_equal(api.bounces_merge(parts), whole, ("three shards", flags))
    t = torch.full((45, 80, 176), 0xAB, dtype=torch.uint8, device="cuda")
    acc = np.zeros(45 * 80 * 176, np.uint8)
    for rank in range(2):
        with api.Renderer(s, flags=flags, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=2) as r:
            assert r.bounces_into(t, 0, n) is t  # (all of it is written: zeros, then this shard's tiles)
            r.sync()
            acc |= t.cpu().numpy().reshape(-1)  # the shards' tiles are disjoint and the rest of either is zero: one tensor filled by both
    assert acc.tobytes() == whole.tobytes()
    t32 = torch.full((45, 80, 44), -1, dtype=torch.int32, device="cuda")
    with api.Renderer(s, flags=flags) as r:
        assert r.bounces_into(t32, 0, n) is t32
        r.sync()
    assert t32.cpu().numpy().tobytes() == whole.tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_two_ranges_of_frames_are_the_whole_ranges_rows(flags):
    d, first = _basic("cornell", flags)
    r = d["r"]
    whole_s, tail_s = r.bounces_samples(0, 16), r.bounces_samples(8, 8)
    assert tail_s.tobytes() == whole_s[8:].tobytes() and d["samples"].tobytes() == whole_s[:8].tobytes()
    a, b, whole = r.bounces(0, 8), r.bounces(8, 8), r.bounces(0, 16)
    _assert_records_equal(a, first, "the result does not depend on what ran before")
    _assert_records_equal(whole, bref.pixel_records(whole_s), "16 frames")
    assert (whole["n"] == 16).all()
    for k in ("n", "length_sum", "capped"):
        assert np.array_equal(a[k] + b[k], whole[k]), k
    assert np.array_equal(a["bucket"]["reached"] + b["bucket"]["reached"], whole["bucket"]["reached"])
    assert np.array_equal(np.maximum(a["length_max"], b["length_max"]), whole["length_max"])


# ---- contexts -------------------------------------------------------------------------------------------------------------------------------------------
def test_an_adaptive_context_and_a_reset_give_the_plain_records():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r:
        even = r.bounces(0, 8)
    with api.Renderer(s) as r:
        r.render(0, 8)
        active = np.indices((3, 4)).sum(0) % 2  # half of the tiles go on
        r.set_active_tiles(active)
        r.render(8, 8)
        assert r.bounces(0, 8).tobytes() == even.tobytes()
        assert sorted(set(r.tile_frames().reshape(-1).tolist())) == [8, 16]  # (the mask was in force, and still is)
    with api.Renderer(s) as r:
        r.bounces(0, 8)
        r.reset()
        assert api._download_result(r, api.lib().rene_download_bounces, (70, 100), abi.BOUNCES_DTYPE).tobytes() == even.tobytes()  # (a reset does not invalidate it)


def test_refusals_that_need_a_device():
    import torch
    r = device("cornell", 0)["r"]
    W, H = r.xres, r.yres
    p = api.bounces_params_default()
    need = api.bounces_bytes(W, H)
    t = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    host = np.zeros(need + 16, np.uint8)
    cases = ((host.ctypes.data, need), (t.data_ptr(), need - 1), (t.data_ptr() + 4, need))  # a host pointer; short; misaligned
    for dst, size in cases:
        with pytest.raises(api.ReneError) as e:
            api._check(api.lib().rene_bounces(r._h, C.byref(p), C.c_void_p(dst), size))
        assert e.value.code == -1, (dst, size)
    assert not t.cpu().numpy().any()  # nothing was launched
    with pytest.raises(ValueError):
        r.bounces_into(torch.zeros(need - 176, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        r.bounces_into(torch.zeros(need // 4, dtype=torch.float32, device="cuda"))
    with pytest.raises((TypeError, ValueError)):
        r.bounces_into(torch.zeros(need, dtype=torch.uint8))  # host memory
    one = np.zeros(1, abi.BOUNCES_SAMPLE_DTYPE)  # more than 2^20 records: refused before the destination is looked at
    p.n_frames = 65536
    assert api.lib().rene_bounces_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"2^20" in api.lib().rene_last_error()
    p.n_frames = 2
    assert api.lib().rene_bounces_samples(r._h, C.byref(p), one.ctypes.data_as(C.c_void_p), 1) == -1 and b"smaller" in api.lib().rene_last_error()
    with api.Renderer(scenes.cornell_fog(32, 32)) as fog:
        for call in (lambda: fog.bounces(0, 2), lambda: fog.bounces_samples(0, 1)):
            with pytest.raises(api.ReneError) as e:
                call()
            assert e.value.code == -4 and "volpath" in str(e.value)  # RENE_ERR_UNSUPPORTED, and the message says why

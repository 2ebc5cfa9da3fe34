"""CPU: rene_plan_memory -- the device memory a context allocates, planned without a GPU.  Chains and version words are sized by the
pixel slots of the tiles a context owns (owned tiles x 1024), so every resolution rene_create accepts has a plan, and a tile shard
pays for its own tiles only."""
import ctypes as C

import pytest

from rene_amd import abi, api, scenes

CHAINS = 8


def _tiles(w, h):
    return ((w + 31) // 32) * ((h + 31) // 32)


def _owned(n_tiles, rank, count):
    return (n_tiles - rank + count - 1) // count if n_tiles > rank else 0


@pytest.mark.parametrize("w,h", [(4096, 2160), (7680, 4320), (16384, 16384)])
def test_unsharded_large_images_are_planned(hip_lib, w, h):
    plan = api.plan_memory(scenes.cornell_box(w, h))
    n_slots = _tiles(w, h) * 1024
    assert plan["chain_bytes"] == CHAINS * 3 * 16 * n_slots
    assert plan["version_bytes"] == CHAINS * 4 * n_slots
    assert plan["image_bytes"] == 3 * w * h * 16
    assert plan["queue_bytes"] == 0
    assert plan["scene_bytes"] > 0
    parts = plan["chain_bytes"] + plan["version_bytes"] + plan["image_bytes"] + plan["scene_bytes"] + plan["queue_bytes"]
    assert parts <= plan["total_bytes"] <= parts + (1 << 20)


def test_tile_shard_plans_its_own_tiles():
    w = h = 16384
    s = scenes.cornell_box(w, h)
    whole = api.plan_memory(s)
    n_tiles = _tiles(w, h)
    total_chain = total_version = 0
    for rank in range(8):
        part = api.plan_memory(s, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=8)
        owned = _owned(n_tiles, rank, 8)
        assert part["chain_bytes"] == CHAINS * 3 * 16 * owned * 1024
        assert part["version_bytes"] == CHAINS * 4 * owned * 1024
        assert part["image_bytes"] == whole["image_bytes"]  # the image handed out is whole on every rank
        total_chain += part["chain_bytes"]
        total_version += part["version_bytes"]
    assert total_chain == whole["chain_bytes"] and total_version == whole["version_bytes"]
    assert whole["chain_bytes"] % 8 == 0 and part["chain_bytes"] * 8 == whole["chain_bytes"]
    # an eighth of a 16384^2 image: ~27 GB planned instead of ~125 GB
    assert 25e9 < part["total_bytes"] < 29e9 and whole["total_bytes"] > 120e9
    # frame shards own every tile
    frames = api.plan_memory(s, shard_mode=abi.SHARD_FRAMES, shard_rank=3, shard_count=8)
    assert frames["chain_bytes"] == whole["chain_bytes"]


def test_ragged_shard_and_wavefront_queues():
    s = scenes.dragon_class(100, 70, 12, 14)  # 4 x 3 tiles, ragged at both edges
    plan = api.plan_memory(s, shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=5)
    assert plan["chain_bytes"] == CHAINS * 3 * 16 * 3 * 1024 and plan["queue_bytes"] == 0  # tiles 1, 6, 11
    wave = api.plan_memory(s, flags=abi.FLAG_WAVEFRONT, shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=5)
    assert wave["chain_bytes"] == plan["chain_bytes"] and wave["queue_bytes"] >= 3 * 1024 * (5 * 16 + 4)
    empty = api.plan_memory(s, shard_mode=abi.SHARD_TILES, shard_rank=13, shard_count=14)  # more ranks than tiles: owns none
    assert empty["chain_bytes"] == 0 and empty["version_bytes"] == 0


def test_caller_owned_framebuffer_plans_no_image():
    s = scenes.cornell_box(4096, 2160)
    plan = api.plan_memory(s, framebuffer_ptr=0x1000)
    assert plan["image_bytes"] == 0
    assert plan["chain_bytes"] == api.plan_memory(s)["chain_bytes"]


def test_refused_like_rene_create(hip_lib):
    s = scenes.cornell_box(16385, 64)
    with pytest.raises(api.ReneError) as e:
        api.plan_memory(s)
    assert e.value.code == -1  # RENE_ERR_INVALID_ARGUMENT
    assert "resolutions above 16384 are not supported" in str(e.value)
    # rene_create refuses the same scene with the same status and message, before it looks for a device
    o = abi.Opts()
    o.struct_size = C.sizeof(abi.Opts)
    h = C.c_void_p()
    plan = abi.MemoryPlan()
    rc_plan = hip_lib.rene_plan_memory(s.to_desc().byref(), C.byref(o), C.byref(plan))
    msg_plan = hip_lib.rene_last_error()
    from conftest import has_gpu
    if has_gpu():
        rc = hip_lib.rene_create(s.to_desc().byref(), C.byref(o), C.byref(h))
        assert rc == rc_plan and hip_lib.rene_last_error() == msg_plan
    assert rc_plan == -1
    with pytest.raises(api.ReneError, match="shard_rank >= shard_count"):
        api.plan_memory(scenes.cornell_box(64, 64), shard_rank=2, shard_count=2)

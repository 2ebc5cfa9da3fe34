"""GPU: the three per-pixel frame-range passes -- geometry, occlusion, direct light -- where what they share (rene_amd/csrc/pixel_pass.h: the
slot -> pixel map and the launch) meets all of them at once: a scene that takes the BVH form on a 3 x 2 tile grid ragged on both edges, unsharded
and as three tile shards.  The other shard tests run the Cornell box, which takes the small-scene form."""
import pytest

import gbuffer_reference as gr
from gbuffer_reference import _assert_records_equal
from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

W, H, FRAMES, SHARDS = 80, 45, 4, 3


def _passes(r):
    return {"gbuffer": r.gbuffer(0, FRAMES), "occlusion": r.occlusion(0, FRAMES), "direct": r.direct(0, FRAMES)}


def test_merged_tile_shards_equal_the_unsharded_records_of_every_pass_on_a_bvh_scene():
    s = scenes.dragon_class(W, H, 48, 52)
    assert not api.pack_info(s).features & abi.FEAT_SMALL  # the BVH instantiations
    with api.Renderer(s) as r:
        whole = _passes(r)
    parts = {name: [] for name in whole}
    for rank in range(SHARDS):
        with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=SHARDS) as r:
            for name, rec in _passes(r).items():
                own = gr.owned_mask(W, H, rank, SHARDS)
                assert (rec["n"][own] == FRAMES).all() and not rec["n"][~own].any(), (name, rank)
                parts[name].append(rec)
    merge = {"gbuffer": api.gbuffer_merge, "occlusion": api.occlusion_merge, "direct": api.direct_merge}
    for name, rec in whole.items():
        assert rec.shape == (H, W) and (rec["n"] == FRAMES).all(), name
        _assert_records_equal(merge[name](parts[name]), rec, name)
    # one pixel map and one primary ray: the three passes count the same hits on every pixel
    assert (whole["gbuffer"]["hits"] == whole["occlusion"]["hits"]).all() and (whole["occlusion"]["hits"] == whole["direct"]["hits"]).all()
    assert whole["gbuffer"]["hits"].any() and (whole["gbuffer"]["hits"] <= FRAMES).all()

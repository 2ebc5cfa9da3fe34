"""CPU: the numpy restatement of the light-group pass's records (tests/lights_reference.py) against api.py's figures on crafted records, bit for
bit, and -- through the CPU oracle -- the ground the GPU tests stand on: a render is the sum of its renders with all but one group of sources
black, and blacking a source leaves every path where it was."""
import numpy as np
import pytest

import lights_reference as lref
import lights_scenes
from rene_amd import abi, api

BITS = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
FRAMES = 8


def _crafted_records():
    """(H, W) = (2, 3) pixel records: plain sums, an unused group, a non-finite value, an unowned pixel (n == 0), one with a single sample."""
    rng = np.random.default_rng(11)
    rec = np.zeros((2, 3), abi.LIGHTS_DTYPE)
    for y in range(2):
        for x in range(3):
            v = rng.uniform(0.0, 4.0, (5, 8, 3)).astype(np.float32)
            v[:, 5] = 0  # nothing maps to group 5
            v[rng.uniform(size=(5, 8)) < 0.4] = 0
            one = lref.pixel_records(lref.crafted(v))
            rec[y, x] = one[0, 0]
    rec["group"]["sum"][0, 1, 2, 1] = np.inf
    rec["group"]["sum"][1, 0, 3, 0] = np.nan
    rec[1, 2] = np.zeros((), abi.LIGHTS_DTYPE)  # a pixel of a tile the context does not own
    single = np.full((1, 8), 0.1, np.float32)
    single[0, 5] = 0
    rec[0, 2] = lref.pixel_records(lref.crafted(single))[0, 0]
    return rec


def test_pixel_records_fold_the_samples_in_frame_order():
    big, small = np.float32(2.0 ** 24), np.float32(1.0)
    v = np.zeros((4, 8), np.float32)
    v[:, 1] = [big, small, small, small]  # ((2^24 + 1) + 1) + 1 stays 2^24 in fp32; any other order of adding gives more
    v[:, 6] = [small, small, small, big]
    s = lref.crafted(v, lit=[1, 1, 0, 1], length=[3, 1, 2, 50], end=[0, 1, 2, 4])
    s["group"]["adds"][:, 0, 0, 1] = [2, 1, 0, 3]
    rec = lref.pixel_records(s)
    assert rec.shape == (1, 1) and rec["n"][0, 0] == 4 and rec["lit"][0, 0] == 3 and not rec["reserved"].any()
    assert rec["group"]["sum"][0, 0, 1, 0] == big and rec["group"]["sum"][0, 0, 6, 0] == np.float32(2.0 ** 24 + 4.0)
    assert rec["group"]["adds"][0, 0].tolist() == [0, 6, 0, 0, 0, 0, 4, 0]
    assert not BITS(rec["group"]["sum"][0, 0, [0, 2, 3, 4, 5, 7]]).any()  # + 0 where nothing was added
    empty = lref.pixel_records(np.zeros((3, 2, 2), abi.LIGHTS_SAMPLE_DTYPE))  # samples of tiles the context does not own
    assert empty.tobytes() == bytes(4 * 144)


def test_sum_mean_mix_and_merge_are_the_apis_bit_for_bit():
    rec = _crafted_records()
    assert (rec["n"] == np.array([[5, 5, 1], [5, 5, 0]])).all()
    with np.errstate(invalid="ignore", over="ignore"):
        assert BITS(api.lights_sum(rec)).tobytes() == BITS(lref.total(rec)).tobytes()
        for g in range(8):
            assert BITS(api.lights_group_mean(rec, g)).tobytes() == BITS(lref.group_mean(rec, g)).tobytes(), g
            assert BITS(api.lights_group_sum(rec, g)).tobytes() == BITS(rec["group"]["sum"][..., g, :]).tobytes(), g
        assert not api.lights_group_mean(rec, 5).any() and not api.lights_group_mean(rec, 0)[1, 2].any()  # the unused group; n == 0
        ones = np.ones(8, np.float32)
        weights = (ones, np.arange(8, dtype=np.float32), np.array([-0.0, 1, -0.0, 2, 0.5, -0.0, 3, 0], np.float32),
                   np.random.default_rng(3).uniform(0, 2, (8, 3)).astype(np.float32), np.array([0, 0, np.inf, 0, 0, 0, 0, 0], np.float32))
        for w in weights:
            got, want = api.lights_mix(rec, w), lref.mix(rec, w)
            assert got.dtype == np.float32 and got.shape == (2, 3, 3)
            assert BITS(got).tobytes() == BITS(want).tobytes(), w
            assert not BITS(got[1, 2]).any()  # n == 0: + 0
        unit = api.lights_mix(rec, ones)
        n = rec["n"].astype(np.float32)[..., None]
        own = (rec["n"] != 0) & np.isfinite(rec["group"]["sum"]).all(axis=(-1, -2))  # (a NaN's payload is nobody's contract)
        assert own.sum() == 3
        assert BITS(unit[own]).tobytes() == BITS((api.lights_sum(rec) / np.where(n == 0, 1, n))[own]).tobytes()  # (1 x is exact)
        # - 0 weights: the product is - 0 and the fold from the left absorbs it wherever a + 0 or a positive term came first
        minus = api.lights_mix(rec, np.array([1, -0.0, -0.0, -0.0, -0.0, -0.0, -0.0, -0.0], np.float32))
        assert BITS(minus[own]).tobytes() == BITS(lref.group_mean(rec, 0)[own]).tobytes()
    for bad in (np.ones(7), np.ones((8, 2)), np.ones((3, 8))):
        with pytest.raises(ValueError):
            api.lights_mix(rec, bad)
    for f in (api.lights_group_sum, api.lights_group_mean):
        with pytest.raises(ValueError):
            f(rec, 8)
    with pytest.raises(TypeError):
        api.lights_sum(np.zeros(3, abi.BOUNCES_DTYPE))
    # merge: the union of disjoint shards, and a refusal where two hold one pixel
    a, b = rec.copy(), rec.copy()
    a[:, 1:] = np.zeros((), abi.LIGHTS_DTYPE)
    b[:, :1] = np.zeros((), abi.LIGHTS_DTYPE)
    assert api.lights_merge([a, b]).tobytes() == lref.merge([a, b]).tobytes() == rec.tobytes()
    with pytest.raises(ValueError):
        api.lights_merge([rec, a])


def _oracle_parts(oracle_mod):
    s = lights_scenes.cornell()
    assert (s.film.xresolution, s.film.yresolution) == (72, 40)
    (inst, dist, bg), used = lights_scenes.default_groups(s)
    assert used == 4 and bg == 0 and dist.tolist() == [1] and inst[lights_scenes.emitting(s)].tolist() == [2, 3]
    full = lref.oracle_only("cornell", lights_scenes.cornell, None, FRAMES, oracle_mod)
    parts = [lref.oracle_only("cornell", lights_scenes.cornell, g, FRAMES, oracle_mod) for g in range(used)]
    return full, parts


def test_the_oracles_full_render_is_the_sum_of_its_groups_and_blacking_leaves_the_paths_alone(oracle_mod):
    """oracle(full) against the sum over g of oracle(only group g lit) on the Cornell scene at 72 x 40 x 8, both summed in doubles: 1e-9
    relative per pixel and channel.  And every counter of a blacked render -- closest-hit, any-hit and emitter queries, paths, bounces, hits, adds
    -- is the full render's: the estimator's draws and throughputs do not depend on a radiance, which is what the GPU tests stand on."""
    full, parts = _oracle_parts(oracle_mod)
    for p in parts:
        for k in ("rays_closest", "rays_shadow", "rays_emitter", "paths", "bounces", "hits", "adds"):
            assert p["stats"][k] == full["stats"][k], k
    want, got = full["doubles"], sum(p["doubles"] for p in parts)
    assert np.isfinite(want).all() and np.isfinite(got).all() and (want >= 0).all() and want.sum() > 0
    rel = np.abs(got - want) / np.where(want == 0, 1.0, want)
    print("oracle(full) against the sum over the groups: largest relative difference", rel.max(), "pixels above 1e-9:", int((rel > 1e-9).any(axis=-1).sum()), "of", rel.shape[0] * rel.shape[1],
          "closest-hit queries:", full["stats"]["rays_closest"])
    assert rel.max() <= 1e-9
    filled = [bool(p["doubles"].any()) for p in parts]
    assert filled == [False, True, True, True]  # a Matte-only Cornell box has no background; the sun and the two lamps all arrive
    assert np.allclose(full["doubles"], full["image"], rtol=1e-5, atol=0)  # (the doubles are the image's radiance)

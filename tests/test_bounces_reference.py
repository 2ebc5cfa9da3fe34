"""CPU: the numpy restatement of the bounce pass's records (tests/bounces_reference.py) on crafted one-pixel sample lists -- the + 0 a sample adds
where it has nothing, an order of additions that shows in fp32, bucket 9's aggregation, the lengths and the cap's count -- the Python helpers
bounces_sum, bounces_depth_mean, bounces_mean_length, bounces_reached and bounces_merge on crafted records, and the yardstick the GPU tests lean
on: the CPU oracle's decomposition by bounce, added up over iterations 0 .. k - 1, IS its render under a cap of k iterations."""
import numpy as np
import pytest

import bounces_reference as bref
from rene_amd import abi, api
from test_gpu_direct import SCENES, capped, scene

TABLE = ("cornell", "dragon", "veach", "zoo")  # the scenes, sizes and frames of tests/test_gpu_direct.py


def _one(*args, **kw):
    return bref.pixel_records(bref.crafted(*args, **kw))[0, 0]


def _row(**at):
    v = np.zeros(10, np.float32)
    for d, x in at.items():
        v[int(d[1:])] = x
    return v


def test_a_sample_adds_plus_zero_where_it_has_nothing():
    """Three samples that end at iterations 1, 3 and 1: buckets 2 and 3 get one value and two + 0s, and the record is what one add per sample gives."""
    r = _one([_row(d0=0.25, d1=1.0), _row(d0=0.5, d2=0.125, d3=2.0), _row(d1=4.0)], reached=[[1, 1] + [0] * 8, [1, 1, 1, 1] + [0] * 6, [1, 1] + [0] * 8],
             end=[bref.MISS, bref.ZERO, bref.PDF])
    assert r["bucket"]["sum"][:, 0].tolist() == [0.75, 5.0, 0.125, 2.0, 0, 0, 0, 0, 0, 0] and not r["bucket"]["sum"][:, 1:].any()
    assert r["bucket"]["reached"].tolist() == [3, 3, 1, 1, 0, 0, 0, 0, 0, 0]
    assert (r["n"], r["length_sum"], r["length_max"], r["capped"]) == (3, 8, 4, 0)
    assert not np.signbit(r["bucket"]["sum"]).any()  # + 0 + (+ 0) is + 0: a bucket nobody reached is the host's zero


def test_the_sums_run_in_frame_order_in_fp32():
    xs = np.float32([1e8, 1.0, 1.0, -1e8, 1.0, 0.5])
    fwd = bck = np.float32(0)
    for x in xs:
        fwd = np.float32(fwd + x)
    for x in xs[::-1]:
        bck = np.float32(bck + x)
    assert fwd == np.float32(1.5) and bck == np.float32(0.0) and xs.sum(dtype=np.float64) == 3.5  # the order shows, and neither is the exact sum
    v = np.zeros((6, 10, 3), np.float32)
    v[:, 4, 0], v[:, 4, 2], v[:, 9, 1] = xs, xs[::-1], xs
    r = _one(v)
    assert r["bucket"]["sum"][4].tolist() == [1.5, 0.0, 0.0] and r["bucket"]["sum"][9].tolist() == [0.0, 1.5, 0.0]


def test_bucket_nine_takes_every_iteration_from_nine_on():
    """A sample's v[9] arrives as ONE value (the sample's own sum over iterations 9 ..), with the iterations counted in reached; the cap's count
    and the longest sample are kept beside it."""
    r = _one([_row(d9=3.0), _row(d8=1.0, d9=0.5), _row(d0=1.0)], reached=[[1] * 9 + [41], [1] * 9 + [4], [1] + [0] * 9],
             end=[bref.CAP, bref.ROULETTE, bref.MISS])
    assert r["bucket"]["reached"].tolist() == [3] + [2] * 8 + [45] and r["bucket"]["sum"][9, 0] == 3.5 and r["bucket"]["sum"][8, 0] == 1.0
    assert (r["n"], r["length_sum"], r["length_max"], r["capped"]) == (3, 50 + 13 + 1, 50, 1)


def test_an_unowned_pixel_is_the_zero_record():
    assert bref.pixel_records(np.zeros((4, 2, 3), abi.BOUNCES_SAMPLE_DTYPE)).tobytes() == bytes(176 * 6)
    assert np.dtype(abi.BOUNCES_DTYPE).itemsize == 176 == np.dtype(abi.BOUNCES_SAMPLE_DTYPE).itemsize


def test_bounces_sum_adds_from_the_left():
    rec = np.zeros((1, 1), abi.BOUNCES_DTYPE)
    rec["bucket"]["sum"][0, 0, :4, 0] = (1e8, -1e8, 1.0, 0.5)
    rec["bucket"]["sum"][0, 0, :4, 2] = (1.0, 1e8, -1e8, 0.5)
    rec["n"], rec["length_sum"] = 2, 7
    rec["bucket"]["reached"][0, 0] = np.arange(10)
    for k, want in ((0, (0, 0)), (1, (1e8, 1.0)), (2, (0, 1e8)), (3, (1.0, 0.0)), (4, (1.5, 0.5)), (10, (1.5, 0.5))):  # ((b0 + b1) + b2) + b3
        got = api.bounces_sum(rec, upto=k)
        assert got.dtype == np.float32 and got.shape == (1, 1, 3) and (got[0, 0, 0], got[0, 0, 2]) == tuple(np.float32(want)), k
        assert np.array_equal(got, bref.sum_upto(rec, k))
    assert np.array_equal(api.bounces_sum(rec), api.bounces_sum(rec, 10))
    assert api.bounces_depth_mean(rec, 0)[0, 0].tolist() == [5e7, 0.0, 0.5] and api.bounces_depth_mean(rec, 3)[0, 0].tolist() == [0.25, 0.0, 0.25]
    assert api.bounces_mean_length(rec).tolist() == [[3.5]] and api.bounces_mean_length(rec).dtype == np.float32
    assert api.bounces_reached(rec).shape == (1, 1, 10) and api.bounces_reached(rec)[0, 0].tolist() == list(range(10))
    rec["n"] = 0  # a pixel no part owns
    assert not api.bounces_depth_mean(rec, 0).any() and not api.bounces_mean_length(rec).any()
    for bad in (lambda: api.bounces_sum(rec, 11), lambda: api.bounces_sum(rec, -1), lambda: api.bounces_depth_mean(rec, 10)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        api.bounces_sum(np.zeros(3, abi.DIRECT_DTYPE))


def test_merge_of_two_disjoint_parts_is_the_whole_and_its_errors():
    rng = np.random.default_rng(5)
    s = np.zeros((3, 2, 4), abi.BOUNCES_SAMPLE_DTYPE)
    s["bucket"]["sum"] = rng.uniform(0, 4, s.shape + (10, 3)).astype(np.float32)
    s["bucket"]["reached"] = rng.integers(0, 3, s.shape + (10,))
    s["n"], s["length"], s["end"] = 1, rng.integers(1, 51, s.shape), rng.integers(0, 5, s.shape)
    full = bref.pixel_records(s)
    assert (full["n"] == 3).all() and np.array_equal(full["capped"], (s["end"] == bref.CAP).sum(axis=0))
    left, right = s.copy(), s.copy()
    left[:, :, 2:] = np.zeros((), s.dtype)  # what the probe of a shard leaves of the pixels it does not own
    right[:, :, :2] = np.zeros((), s.dtype)
    parts = [bref.pixel_records(left), bref.pixel_records(right)]
    assert (parts[0]["n"][:, 2:] == 0).all() and parts[0][:, 2:].tobytes() == bytes(176 * 4)
    assert api.bounces_merge(parts).tobytes() == full.tobytes() and api.bounces_merge(parts[::-1]).tobytes() == full.tobytes()
    with pytest.raises(ValueError):
        api.bounces_merge([parts[0], parts[0]])  # two parts hold the same pixel
    with pytest.raises(ValueError):
        api.bounces_merge([])
    with pytest.raises(ValueError):
        api.bounces_merge([parts[0], parts[1][:1]])
    with pytest.raises(TypeError):
        api.bounces_merge([np.zeros((2, 4), abi.DIRECT_DTYPE)])


@pytest.mark.parametrize("name", TABLE)
def test_the_oracles_cumulative_decomposition_is_its_capped_render(name, oracle_mod):
    """Branches 0 + 1 of iterations 0 .. k - 1 against the depth_cap = k render of the same frames, k = 1, 2, 3, 5, and all ten buckets against
    the uncapped render: 1e-6 (1 + |x|) per component.  (The decomposition adds in fp64 and the image in fp32, a handful of adds per pixel and
    iteration: some 2^-24 apiece.)  Which buckets the scene fills is asserted too: a decomposition that kept nothing would pass the rest."""
    dec = bref.decomposition(name, scene(name), SCENES[name][1], oracle_mod)
    for k in (1, 2, 3, 5):
        got, want = bref.cumulative(dec, k), capped(name, k, oracle_mod)
        fin = np.isfinite(want) & np.isfinite(got)
        err = np.abs(np.where(fin, got - want, 0)) / (1 + np.abs(np.where(fin, want, 0)))
        print(name, "cap", k, "largest error relative to 1 + |x|:", float(err.max()), "non-finite components:", int((~fin).sum()))
        assert fin.mean() > 0.99 and err.max() <= 1e-6, (name, k)
    got, want = bref.cumulative(dec, 10), dec["image"]
    fin = np.isfinite(want) & np.isfinite(got)
    err = np.abs(np.where(fin, got - want, 0)) / (1 + np.abs(np.where(fin, want, 0)))
    print(name, "uncapped, largest error relative to 1 + |x|:", float(err.max()))
    assert fin.mean() > 0.99 and err.max() <= 1e-6, name
    filled = [d for d in range(10) if np.nan_to_num(dec["layers"][d]).any()]
    print(name, "buckets filled:", filled)
    want_filled = {"cornell": [0, 1, 2, 3, 4, 5, 6, 7, 9], "dragon": list(range(10)), "zoo": list(range(10)), "veach": [0, 1, 2, 3]}[name]
    assert filled == want_filled, (name, filled)


def test_the_oracles_deep_paths_are_cut_by_a_cap_of_thirteen(oracle_mod):
    """emit_fusion_scenes.deep_paths(32, 32), 8 frames: the closest-hit queries under caps 13, 14, 20 and 50 -- iteration 13 is reached and none
    beyond, so a cap of 13 cuts real paths and the roulette at i > 12 is taken."""
    import emit_fusion_scenes
    s = emit_fusion_scenes.deep_paths(32, 32)
    rays = {}
    for cap in (13, 14, 20, 50):
        o = oracle_mod.Oracle(s)
        o.set_experiment(depth_cap=cap)
        o.render(0, 8)
        rays[cap] = o.stats().as_dict()["rays_closest"]
    print("deep_paths, rays_closest by cap:", rays)
    assert rays == {13: 32142, 14: 32285, 20: 32285, 50: 32285}

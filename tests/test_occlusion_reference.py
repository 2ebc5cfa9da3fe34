"""CPU: the numpy restatement of the occlusion pass (tests/occlusion_reference.py) on crafted one-pixel sample lists -- all misses, a mix, a hit
that casts nothing -- its fp64 direction against values worked out by hand, and the Python helpers occlusion_ao, occlusion_bent and
occlusion_merge on crafted records."""
import numpy as np
import pytest

import occlusion_reference as oref
from rene_amd import abi, api

M, O, X, N3 = oref.MISS, oref.OPEN, oref.OCCLUDED, oref.NO_RAY


def _one(states, ws=None, **kw):
    return oref.aggregate(oref.crafted(states, ws), **kw)[0, 0]


def test_all_misses():
    r = _one([[M, M], [M, M], [M, M]])
    assert (r["hits"], r["rays"], r["occluded"], r["n"], r["reserved"]) == (0, 0, 0, 3, 0) and not r["bent_sum"].any()
    rec = np.array([r])
    assert api.occlusion_ao(rec)[0] == 1 and not api.occlusion_bent(rec).any()


def test_a_mix_counts_per_sample_and_per_ray_and_sums_the_open_directions_only():
    ws = np.zeros((4, 2, 3), np.float32)
    ws[0] = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    ws[2] = [[0.0, 0.0, 0.5], [0.25, 0.0, 0.0]]
    ws[3] = [[0.0, -1.0, 0.0], [0.0, 0.0, 9.0]]
    r = _one([[O, X], [M, M], [O, O], [X, X]], ws)
    # frames 0, 2 and 3 hit: 3 samples, 6 rays, of them [0][1], [3][0], [3][1] occluded; open: (1, 0, 0), (0, 0, 0.5), (0.25, 0, 0)
    assert (r["hits"], r["rays"], r["occluded"], r["n"]) == (3, 6, 3, 4)
    assert r["bent_sum"].tolist() == [1.25, 0.0, 0.5]
    rec = np.array([r])
    assert api.occlusion_ao(rec)[0] == np.float32(0.5)
    length = np.sqrt(np.float32(1.25) * np.float32(1.25) + np.float32(0.5) * np.float32(0.5))
    assert api.occlusion_bent(rec)[0].tolist() == [np.float32(1.25) / length, 0.0, np.float32(0.5) / length]


def test_the_bent_sum_runs_in_frame_and_ray_order_in_fp32():
    xs = np.float32([[1e8, 1.0], [1.0, -1e8], [1.0, 0.5]])
    ws = np.zeros((3, 2, 3), np.float32)
    ws[..., 0] = xs
    r = _one([[O, O], [O, O], [O, O]], ws)
    want = np.float32(0)
    for x in xs.reshape(-1):
        want = np.float32(want + x)  # (1e8 swallows the 1.0s: the order shows)
    assert r["bent_sum"][0] == want == np.float32(1.5) and xs.sum(dtype=np.float64) == 3.5


def test_a_hit_that_casts_nothing_counts_in_hits_alone():
    r = _one([[N3, N3, N3], [O, X, O]])
    assert (r["hits"], r["rays"], r["occluded"], r["n"]) == (2, 3, 1, 2) and r["bent_sum"].tolist() == [0.0, 0.0, 2.0]
    r = _one([[N3], [N3]])
    assert (r["hits"], r["rays"], r["occluded"]) == (2, 0, 0)
    assert api.occlusion_ao(np.array([r]))[0] == 1  # rays == 0


def test_an_unowned_pixel_is_the_zero_record():
    z = oref.aggregate(oref.crafted([[O], [X]]), owned=np.zeros((1, 1), bool))
    assert z.tobytes() == bytes(32)


def test_the_direction_by_hand():
    # n = +z: |x| > |y| is false (a tie), u = (0, z, -y) / sqrt(y^2 + z^2) = (0, 1, 0), v = n x u = (-1, 0, 0)
    n = np.float64([0.0, 0.0, 1.0])
    d = oref.direction(n, 0.0, 0.25)  # local (0.5, 0, sqrt(0.75)) -> 0.5 u + sqrt(0.75) n
    assert np.allclose(d, [0.0, 0.5, np.sqrt(0.75)], atol=1e-15)
    d = oref.direction(n, 0.25, 1.0)  # local (0, 1, 0) -> v
    assert np.allclose(d, [-1.0, 0.0, 0.0], atol=1e-15)
    # n = +x: the first form, u = (-z, 0, x) / sqrt(x^2 + z^2) = (0, 0, 1), v = n x u = (0, -1, 0)
    d = oref.direction(np.float64([1.0, 0.0, 0.0]), 0.5, 0.64)  # local (-0.8, 0, 0.6)
    assert np.allclose(d, [0.6, 0.0, -0.8], atol=1e-15)
    # shapes, unit length and the hemisphere of n
    rng = np.random.default_rng(5)
    ns = rng.normal(size=(7, 11, 3))
    ns /= np.linalg.norm(ns, axis=-1, keepdims=True)
    r1, r2 = rng.uniform(size=(7, 11)), rng.uniform(size=(7, 11))
    d = oref.direction(ns, r1, r2)
    assert d.shape == (7, 11, 3) and np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-12)
    assert np.allclose((d * ns).sum(-1), np.sqrt(1.0 - r2), atol=1e-12)  # the cosine to n is the local z


def test_merge_and_helpers():
    rng = np.random.default_rng(2)
    s = np.zeros((3, 2, 2, 4), abi.OCCLUSION_SAMPLE_DTYPE)
    s["state"] = rng.integers(1, 3, s.shape)
    s["state"][:, :, 0, 0] = M
    s["state"][1, :, 1, 1] = N3
    s["w"] = rng.normal(size=s.shape + (3,)).astype(np.float32)
    full = oref.aggregate(s)
    left = np.zeros((2, 4), bool)
    left[:, :2] = True
    parts = [oref.aggregate(s, owned=left), oref.aggregate(s, owned=~left)]
    assert api.occlusion_merge(parts).tobytes() == full.tobytes() and api.occlusion_merge(parts[::-1]).tobytes() == full.tobytes()
    with pytest.raises(ValueError):
        api.occlusion_merge([parts[0], parts[0]])
    with pytest.raises(ValueError):
        api.occlusion_merge([])
    with pytest.raises(TypeError):
        api.occlusion_ao(np.zeros(3, abi.GBUFFER_DTYPE))
    ao, bent = api.occlusion_ao(full), api.occlusion_bent(full)
    assert ao.dtype == np.float32 and bent.dtype == np.float32 and bent.shape == (2, 4, 3)
    assert ao[0, 0] == 1 and not bent[0, 0].any() and full["hits"][0, 0] == 0
    assert full["hits"][1, 1] == 3 and full["rays"][1, 1] == 4
    want = np.float32(1) - full["occluded"].astype(np.float32) / np.maximum(full["rays"], 1).astype(np.float32)
    assert np.array_equal(ao, want)
    some = (full["bent_sum"] != 0).any(-1)
    assert some.sum() >= 6 and np.allclose(np.linalg.norm(bent[some], axis=-1), 1.0, atol=1e-6) and not bent[~some].any()
    assert api.occlusion_ao(parts[0])[0, 3] == 1  # n == 0: nothing was cast

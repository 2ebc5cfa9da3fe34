"""CPU: the numpy restatement of the direct-light pass's sums (tests/direct_reference.py) on crafted one-pixel sample lists -- a missed pixel, an
order of additions that shows in fp32, an unowned pixel -- and the Python helpers direct_sum, direct_mean, direct_merge and indirect_mean on
crafted records."""
import numpy as np
import pytest

import direct_reference as dref
from rene_amd import abi, api

M, L, B, P, EP, EZ = dref.MISS, dref.LIGHT, dref.BSDF, dref.PLAIN, dref.ENDED_PDF, dref.ENDED_ZERO


def _one(*args, **kw):
    return dref.aggregate(dref.crafted(*args), **kw)[0, 0]


def test_a_missed_pixel_has_no_hits_and_only_seen():
    r = _one([M, M, M], [[0.25, 0.5, 1.0]] * 3)
    assert (r["hits"], r["n"], r["reserved"]) == (0, 3, 0)
    assert r["seen"].tolist() == [0.75, 1.5, 3.0] and not r["distant"].any() and not r["sampled"].any()
    rec = np.array([r])
    assert api.direct_sum(rec)[0].tolist() == [0.75, 1.5, 3.0] and api.direct_mean(rec)[0].tolist() == [0.25, 0.5, 1.0]


def test_every_state_but_a_miss_is_a_hit():
    r = _one([L, B, P, EP, EZ, M], None, [[1, 0, 0]] * 6, [[0, 2, 0]] * 6)
    assert (r["hits"], r["n"]) == (5, 6) and r["distant"].tolist() == [6.0, 0.0, 0.0] and r["sampled"].tolist() == [0.0, 12.0, 0.0]


def test_the_sums_run_in_frame_order_in_fp32():
    xs = np.float32([1e8, 1.0, 1.0, -1e8, 1.0, 0.5])
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(1.0)
    assert np.float32(np.float32(a + b) + c) != np.float32(a + np.float32(b + c))  # (a + b) + c != a + (b + c): the order shows
    v = np.zeros((6, 3), np.float32)
    v[:, 0] = xs
    v[:, 2] = xs[::-1]
    want0 = want2 = np.float32(0)
    for x in xs:
        want0 = np.float32(want0 + x)
    for x in xs[::-1]:
        want2 = np.float32(want2 + x)
    for field in range(3):
        args = [None, None, None]
        args[field] = v
        r = _one([P] * 6, *args)
        got = r[("seen", "distant", "sampled")[field]]
        assert got[0] == want0 == np.float32(1.5) and got[2] == want2 == np.float32(0.0) and got[1] == 0
    assert xs.sum(dtype=np.float64) == 3.5  # neither is the exact sum


def test_an_unowned_pixel_is_the_zero_record():
    z = dref.aggregate(dref.crafted([L, B], [[1, 1, 1]] * 2), owned=np.zeros((1, 1), bool))
    assert z.tobytes() == bytes(48)


def _random_samples(shape, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros(shape, abi.DIRECT_SAMPLE_DTYPE)
    s["state"] = rng.integers(0, 6, shape)
    for k in ("seen", "distant", "sampled"):
        s[k] = rng.uniform(0, 4, shape + (3,)).astype(np.float32)
    return s


def test_direct_sum_adds_in_the_headers_order():
    rec = np.zeros(1, abi.DIRECT_DTYPE)
    rec["seen"][0, 0], rec["distant"][0, 0], rec["sampled"][0, 0], rec["n"] = 1e8, -1e8, 1.0, 2
    assert api.direct_sum(rec)[0, 0] == 1.0  # (seen + distant) + sampled; seen + (distant + sampled) is 0
    assert api.direct_mean(rec)[0, 0] == 0.5 and api.direct_sum(rec).dtype == np.float32 and api.direct_mean(rec).dtype == np.float32


def test_merge_of_two_disjoint_parts_is_the_whole():
    s = _random_samples((3, 2, 4), 2)
    full = dref.aggregate(s)
    left = np.zeros((2, 4), bool)
    left[:, :2] = True
    parts = [dref.aggregate(s, owned=left), dref.aggregate(s, owned=~left)]
    assert api.direct_merge(parts).tobytes() == full.tobytes() and api.direct_merge(parts[::-1]).tobytes() == full.tobytes()
    assert (parts[0]["n"][:, 2:] == 0).all() and not api.direct_mean(parts[0])[:, 2:].any()
    with pytest.raises(ValueError):
        api.direct_merge([parts[0], parts[0]])
    with pytest.raises(ValueError):
        api.direct_merge([])
    with pytest.raises(TypeError):
        api.direct_sum(np.zeros(3, abi.OCCLUSION_DTYPE))


def test_indirect_mean_on_a_hand_made_pair():
    rec = np.zeros((1, 2), abi.DIRECT_DTYPE)
    rec["seen"][0, 0], rec["distant"][0, 0], rec["sampled"][0, 0], rec["n"][0, 0] = (1, 0, 0), (0, 2, 0), (0.5, 0.5, 0.5), 4
    beauty = np.zeros((1, 2, 4), np.float32)  # a layer as download() hands it out, with its fourth channel
    beauty[0, 0] = (3.5, 4.5, 0.5, 9.0)
    beauty[0, 1] = (7.0, 7.0, 7.0, 9.0)  # (an unowned pixel: n == 0)
    got = api.indirect_mean(beauty, rec)
    assert got.dtype == np.float32 and got.shape == (1, 2, 3)
    assert got[0, 0].tolist() == [0.5, 0.5, 0.0] and not got[0, 1].any()
    assert np.array_equal(api.indirect_mean(beauty[..., :3], rec), got)
    assert np.array_equal(api.direct_mean(rec)[0, 0] + got[0, 0], beauty[0, 0, :3] / np.float32(4))
    with pytest.raises(ValueError):
        api.indirect_mean(np.zeros((2, 2, 3), np.float32), rec)

"""-m gpu: every render_kernel / render_kernel_wf instantiation of the build (tests/kernel_matrix.py), on a 77 x 45 film.

- The launch log (RENE_TEST_KERNEL_LOG) names exactly the kernel kernel_matrix.expected_kernel restates from the dispatchers, and
  the logs of the whole matrix name every render kernel in *.res.
- A counting variant (RENE_FLAG_COUNTERS) renders 16 frames in two calls (9 + 7) and matches the oracle: radiance at T1 with the
  tolerance of its material class and a floor of a few pixels (one forked path must not fail a film of 3 465 pixels), mean radiance
  within 1e-3, the first-hit layers, and the ray counters.
- Every production variant (counters off; first-hit layers on or off; instance and light tables in LDS or in global memory) equals
  its counting twin bit for bit in radiance and first-hit layers: COUNT guards only counter updates (render_wf.inc, device_code.inc).
  Without first-hit layers (RENE_FLAG_NO_AOV) layers 1 and 2 stay zero.
- Film shapes down to the smallest film rene_create accepts, and tile shards of the ragged film (6 tiles) over 4 and 8 ranks, on the
  item loop, the while-while kernel, two restart kernels and the volpath restart kernel."""

import numpy as np
import pytest

import kernel_matrix as km
from rene_amd import abi, api
from test_gpu_parity import aov_check, t1_check

pytestmark = pytest.mark.gpu

CALLS = (9, 7)
FRAMES = sum(CALLS)
FLOOR_PIXELS = 4
KEYS = ("rays_closest", "rays_emitter", "rays_shadow", "hits", "adds")
_LOGGED = {}  # catalogue entry -> the kernels its launches logged (test_the_logs_name_every_render_kernel_of_the_build)


@pytest.fixture
def log(tmp_path, monkeypatch):
    path = str(tmp_path / "kernels.log")
    monkeypatch.setenv("RENE_TEST_KERNEL_LOG", path)
    return path


def _render(scene, flags, log, monkeypatch, no_lds_tables=False, **opts):
    """16 frames in two calls: the three layers, the counters and the kernel of every launch."""
    if no_lds_tables:
        monkeypatch.setenv("RENE_NO_LDS_TABLES", "1")
    else:
        monkeypatch.delenv("RENE_NO_LDS_TABLES", raising=False)
    km.read_log(log)
    with api.Renderer(scene, flags=flags, **opts) as r:
        f0 = 0
        for n in CALLS:
            r.render(f0, n)
            f0 += n
        imgs = [r.download(l) for l in range(3)]
        st = r.stats().as_dict()
    names = km.read_log(log)
    assert len(names) == st["launches"], (names, st["launches"])
    return imgs, st, names


def _oracle(scene, oracle_mod):
    o = oracle_mod.Oracle(scene)
    o.render(0, FRAMES, threads=16)
    return [o.download(l) for l in range(3)], o.stats().as_dict()


def _against_the_oracle(g, sg, o, so, cls, mean=True, aov_frac=5e-3):
    frac, relmse, ctol = km.TOL[cls]
    floor = FLOOR_PIXELS / (g[0].shape[0] * g[0].shape[1])
    assert sg["paths"] == so["paths"]
    for k in KEYS:
        assert abs(sg[k] - so[k]) <= ctol * so[k] + 4, (k, sg[k], so[k])
    g0, o0 = g[0], o[0]
    assert np.isfinite(g0).all() == np.isfinite(o0).all()
    fin = np.isfinite(g0).all(axis=2) & np.isfinite(o0).all(axis=2)
    t1_check(np.where(fin[..., None], g0, 0), np.where(fin[..., None], o0, 0), frac=max(frac, floor), relmse=relmse)
    for l in (1, 2):
        aov_check(g[l], o[l], atol=5e-5 * FRAMES, frac=max(aov_frac, floor))
    if mean:  # (over the pixels but the floor's few that differ most: one path forked at glass moves the mean of 3 465 by 1e-3)
        keep = fin.copy()
        keep.reshape(-1)[np.argsort(np.abs(g0 - o0).sum(axis=2).reshape(-1))[-FLOOR_PIXELS:]] = False
        assert abs(float(g0[keep].sum() / o0[keep].sum()) - 1) < 1e-3


@pytest.mark.parametrize("name", [e.name for e in km.CATALOGUE])
def test_every_instantiation_against_the_oracle_and_its_counting_twin(name, oracle_mod, log, monkeypatch):
    e = km.BY_NAME[name]
    s = e.build()
    info = api.pack_info(s)
    ref, so = _oracle(s, oracle_mod)
    out, logged = {}, set()
    for v in km.VARIANTS[e.family]:
        g, sg, names = _render(s, v.flags, log, monkeypatch, v.no_lds_tables)
        want = km.expected_kernel(info, v.flags, v.no_lds_tables)
        assert names and set(names) == {want}, (v.name, names, want)
        logged.add(want)
        if v.twin is None:
            _against_the_oracle(g, sg, ref, so, e.cls)
            assert sg["hits"] > 0 and g[0].sum() > 0
        else:
            t, st = out[v.twin]
            assert np.array_equal(g[0], t[0]), (v.name, v.twin, int((g[0] != t[0]).sum()))
            for l in (1, 2):
                if v.flags & abi.FLAG_NO_AOV:
                    assert not g[l].any(), (v.name, l)
                else:
                    assert np.array_equal(g[l], t[l]), (v.name, v.twin, l)
            assert sg["paths"] == st["paths"]
        out[v.name] = (g, sg)
    _LOGGED[name] = logged


def test_the_logs_name_every_render_kernel_of_the_build():
    """After the matrix above (file order): the kernels its launches logged are every render kernel in *.res."""
    if len(_LOGGED) < len(km.CATALOGUE):
        pytest.skip("needs the whole matrix of this module in the same session")
    res = km.res_kernel_names()
    if res is None:
        pytest.skip("rene_amd/csrc/*.res missing")
    logged = set().union(*_LOGGED.values())
    assert logged == res, {"not launched": sorted(res - logged), "not compiled": sorted(logged - res)}


# item loop 64, while-while 8, restart 2056 and 63, volpath restart 136
EDGES = [("cornell", 0), ("matte-deep+emitter", abi.FLAG_NO_RESTART), ("matte-deep+sun", 0), ("plastic-uber-deep", 0), ("fog-deep", 0)]
EDGE_IDS = ["item-64", "ww-8", "restart-2056", "restart-63", "vol-restart-136"]


@pytest.mark.parametrize("w,h", [(2, 2), (2, 45), (77, 2), (33, 33)])
@pytest.mark.parametrize("name,extra", EDGES, ids=EDGE_IDS)
def test_film_shapes_against_the_oracle(name, extra, w, h, oracle_mod, log, monkeypatch):
    """2 x 2 is the smallest film rene_create accepts; one- and two-tile-wide strips; a film one texel past a tile."""
    e = km.BY_NAME[name]
    s = e.build().with_resolution(w, h)
    info = api.pack_info(s)
    flags = abi.FLAG_COUNTERS | extra
    ref, so = _oracle(s, oracle_mod)
    g, sg, names = _render(s, flags, log, monkeypatch)
    assert names and set(names) == {km.expected_kernel(info, flags)}
    assert sg["paths"] == w * h * FRAMES
    _against_the_oracle(g, sg, ref, so, e.cls, mean=False)


@pytest.mark.parametrize("name,extra", EDGES, ids=EDGE_IDS)
def test_tile_shards_of_the_ragged_film(name, extra, log, monkeypatch):
    """77 x 45 is 3 x 2 tiles.  Over 4 and 8 ranks (the production variant): ranks 6 and 7 own no tile -- no launch, a zero image,
    no path -- and the ranks' three layers add up to the unsharded ones bit for bit."""
    s = km.BY_NAME[name].build()
    want = km.expected_kernel(api.pack_info(s), extra)
    whole, st, names = _render(s, extra, log, monkeypatch)
    assert names and set(names) == {want}
    for count in (4, 8):
        acc = [np.zeros_like(x) for x in whole]
        paths = 0
        for rank in range(count):
            g, sg, names = _render(s, extra, log, monkeypatch, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=count)
            if rank >= 6:
                assert sg["paths"] == 0 and not names and not any(x.any() for x in g), (count, rank)
            else:
                assert sg["paths"] > 0 and names and set(names) == {want}, (count, rank, names)
            paths += sg["paths"]
            for l in range(3):
                acc[l] += g[l]
        assert paths == st["paths"]
        for l in range(3):
            assert np.array_equal(acc[l], whole[l]), (count, l)

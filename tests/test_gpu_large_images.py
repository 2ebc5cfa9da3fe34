"""-m gpu: images beyond 2^23 pixel slots on one context, and tile shards that hold chains for their own tiles only.

Every kernel family renders 4096 x 2160 (8704 tiles, 8.9 M slots) unsharded; its tile shards add up to it bit for bit, and so do
the shards of 7680 x 4320.  A 16384^2 image is rendered only as tile shards (an unsharded context would hold ~125 GB of a shared
card), compared on the device through caller-owned framebuffers."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from rene_amd import abi, api, scenes
from test_gpu_parity import aov_check, t1_check

pytestmark = pytest.mark.gpu


def _layers(r):
    return [r.download(l) for l in range(3)]


def _shard_sum(scene, n, frames, flags=0):
    total = None
    for rank in range(n):
        with api.Renderer(scene, flags=flags, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=n) as r:
            r.render(0, frames)
            got = _layers(r)
        total = got if total is None else [a + b for a, b in zip(total, got)]
    return total


def _owned_mask(w, h, rank, count):
    tiles_x = (w + 31) // 32
    ty, tx = np.meshgrid(np.arange(h) // 32, np.arange(w) // 32, indexing="ij")
    return (ty * tiles_x + tx) % count == rank


def test_cornell_4k_unsharded_matches_shards_and_oracle(oracle_mod):
    w, h = 4096, 2160
    s = scenes.cornell_box(w, h)
    with api.Renderer(s) as r:
        r.render(0, 4)
        whole = _layers(r)
        assert r.stats().as_dict()["paths"] == w * h * 4
    for a, b in zip(whole, _shard_sum(s, 3, 4)):
        assert np.array_equal(a, b)
    # one frame against the oracle on the tiles of rank 15 of a 16-way cut (the last column of tiles and the bottom-right tile)
    with api.Renderer(s) as r:
        r.render(0, 1)
        one = _layers(r)
    o = oracle_mod.Oracle(s)
    o.render(0, 1, threads=16, shard_mode=abi.SHARD_TILES, shard_rank=15, shard_count=16)
    m = _owned_mask(w, h, 15, 16)
    assert m[h - 1, w - 1] and m[0, w - 1]
    t1_check(one[0][m], o.download(0)[m])
    aov_check(one[1][m], o.download(1)[m], atol=2e-5)
    aov_check(one[2][m], o.download(2)[m], atol=1e-6)


def test_restart_kernel_4k_shards_cuts_and_families():
    w, h = 4096, 2160
    s = scenes.dragon_class(w, h, 80, 88)
    with api.Renderer(s) as r:
        r.render(0, 8)
        whole = _layers(r)
        r.reset()
        r.render(0, 3)
        r.render(3, 5)
        cut = _layers(r)
    for a, b in zip(whole, cut):
        assert np.array_equal(a, b)
    for a, b in zip(whole, _shard_sum(s, 3, 8)):
        assert np.array_equal(a, b)
    for flags in (abi.FLAG_NO_RESTART, abi.FLAG_WAVEFRONT):
        with api.Renderer(s, flags=flags) as r:
            r.render(0, 8)
            for a, b in zip(whole, _layers(r)):
                assert np.array_equal(a, b), flags


def test_volpath_above_2_23_slots_matches_shards():
    s = scenes.cornell_fog(3072, 3072)  # 9216 tiles: 9.4 M slots
    with api.Renderer(s) as r:
        r.render(0, 2)
        whole = _layers(r)
    assert whole[0].max() > 0
    for a, b in zip(whole, _shard_sum(s, 3, 2)):
        assert np.array_equal(a, b)


def _device_fb(w, h):
    import torch
    return torch.zeros((3, h, w, 4), dtype=torch.float32, device="cuda")


def test_8k_unsharded_matches_four_shards():
    import torch
    w, h = 7680, 4320
    s = scenes.cornell_box(w, h)
    whole, parts = _device_fb(w, h), _device_fb(w, h)
    with api.Renderer(s, framebuffer_ptr=whole.data_ptr()) as r:
        r.render(0, 2)
        r.sync()
    # the four shards' tiles are disjoint: one framebuffer of all four is their sum (every context is created before any renders:
    # rene_create clears the framebuffer it is given)
    rs = [api.Renderer(s, framebuffer_ptr=parts.data_ptr(), shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=4) for k in range(4)]
    try:
        for r in rs:
            r.render(0, 2)
        for r in rs:
            r.sync()
    finally:
        for r in rs:
            r.close()
    torch.cuda.synchronize()
    assert float(whole[0].max()) > 0
    assert torch.equal(whole, parts)


def test_16k_tile_shard_renders_its_tiles_only():
    import torch
    w = h = 16384
    s = scenes.cornell_box(w, h)
    a = _device_fb(w, h)
    with api.Renderer(s, framebuffer_ptr=a.data_ptr(), shard_mode=abi.SHARD_TILES, shard_rank=7, shard_count=8) as r:
        r.render(0, 2)
        r.sync()
        st = r.stats().as_dict()
    assert st["paths"] == (w * h // 8) * 2
    torch.cuda.synchronize()
    # 512 tiles per row: rank 7 of 8 owns every tile column tx % 8 == 7, the bottom-right tile (x, y = 16383) among them
    for layer in range(3):
        v = a[layer].view(h, 64, 8, 32, 4)
        assert int(torch.count_nonzero(v[:, :, :7])) == 0, layer  # nothing written outside its tiles
        assert int(torch.count_nonzero(v[..., 3])) == 0  # (the handed-out image's alpha is 0)
    assert int(torch.count_nonzero(a[:, h - 32:, w - 32:, :3])) > 0  # the bottom-right tile is rendered
    assert int(torch.count_nonzero(a[1].view(h, 64, 8, 32, 4)[:, :, 7, :, :3])) > 0
    # ranks 7 and 15 of a 16-way cut own the same tiles between them
    b = _device_fb(w, h)
    rs = [api.Renderer(s, framebuffer_ptr=b.data_ptr(), shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=16) for k in (7, 15)]
    try:
        for r in rs:
            r.render(0, 2)
        for r in rs:
            r.sync()
    finally:
        for r in rs:
            r.close()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_dropped_item_report_names_pixel_and_chain():
    """The traversal-restart kernels report a dropped item as x | y << 14 | chain << 28, like the item-loop kernels: the first
    dropped pixel lies inside the image and its chain is printed (RENE_TEST_DROP drops items in software; nothing faults)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from rene_amd import api, scenes\n"
            "with api.Renderer(scenes.dragon_class(160, 90, 40, 44)) as r:\n"
            "    r.render(0, 24); r.sync()\n" % ROOT)
    env = dict(os.environ, RENE_DEBUG="1", RENE_TEST_DROP="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = next(l for l in p.stderr.splitlines() if "work items were dropped" in l)
    first = line.split("the first: pixel (")[1]
    x, y = (int(v) for v in first.split(")")[0].split(","))
    chain = int(first.split("chain ")[1].split(",")[0])
    assert 0 <= x < 160 and 0 <= y < 90, line
    assert 0 <= chain < 8, line


def test_cli_renders_4k(hip_lib, tmp_path):
    cli = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
    out = tmp_path / "cornell-4k.png"
    scene = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    env = dict(os.environ, RENE_DEBUG="1")
    p = subprocess.run([cli, scene, "--width", "4096", "--height", "2160", "--spp", "2", "--out", str(out)], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "memory plan" in p.stderr
    data = out.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    assert struct.unpack(">II", data[16:24]) == (4096, 2160)

"""GPU: the multi-channel OpenEXR output on the device (rene_output_exr, include/rene_hip.h).  Everything here compares BYTES: the file of a rendered
job with every layer against the header and a numpy pack of what the downloads hand out (tests/exr_reference.py, through the independent writer of
tests/test_images.py), odd and even widths, crafted chains at the edges of the half format against the host function, an adaptive context, three
tile shards into one tensor, that the call changes nothing it reads, the destination's validation and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_reference as ar
import chain_reference as cr
import exr_reference as er
from conftest import ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
W, H = 77, 45          # odd W, ragged tiles: 3 x 2 of them
FRAMES = 5
GB_FIRST, GB_FRAMES = 3, 5  # the geometry pass's frames, tests/gbuffer_reference.py's
GEOMETRY = abi.EXR_ALPHA | abi.EXR_DEPTH | abi.EXR_POSITION | abi.EXR_IDS
NO_DENOISED = abi.EXR_ALL & ~abi.EXR_DENOISED


def records(r):
    """The library-owned records of the context's last gbuffer(), without another pass."""
    return api._download_result(r, api.lib().rene_download_gbuffer, (r.yres, r.xres), abi.GBUFFER_DTYPE)


def numpy_file(r, mask, beauty="radiance"):
    """The header and a numpy pack of the context's downloads."""
    pl = dict(albedo=r.download_mean(2), normal=r.download_mean(1))
    if mask & abi.EXR_DENOISED or beauty == "denoised_mean":
        pl["denoised"] = r.download_denoised(abi.DENOISED_MEAN)
    pl["beauty"] = {"radiance": lambda: r.download_mean(0), "denoised_mean": lambda: pl["denoised"], "robust": lambda: r.download_robust()}[beauty]()
    if mask & GEOMETRY:
        pl.update(er.gbuffer_planes(records(r)))
    data = er.file_bytes(mask, r.yres, r.xres, **pl)
    head = api.exr_layout(r.xres, r.yres, mask)[0]
    assert api.exr_header(r.xres, r.yres, mask) == data[:head]
    return data


def same(got, want, label):
    assert len(got) == len(want), (label, len(got), len(want))
    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert bad.size == 0, (label, len(bad), bad[:8].tolist())


def code(fn):
    with pytest.raises(api.ReneError) as e:
        fn()
    assert str(e.value).split(": ", 1)[1].strip()  # a message
    return e.value.code


@pytest.fixture(scope="module")
def job():
    """Cornell 77 x 45: five frames, the geometry pass over frames 3 .. 7, denoised."""
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.render(0, FRAMES)
        r.gbuffer(GB_FIRST, GB_FRAMES)
        r.denoise()
        yield r


def test_every_layer_of_a_rendered_job(job, tmp_path):
    r = job
    want = numpy_file(r, abi.EXR_ALL)
    path = tmp_path / "all.exr"
    got = r.exr(path=str(path), layers=abi.EXR_ALL)
    same(got, want, "every layer")
    assert path.read_bytes() == got
    ptr, n = r.exr_buffer()
    assert ptr and n == api.exr_layout(W, H, abi.EXR_ALL)[1] == H * (8 + W * 66)
    w, h, ch = er.parse(got)
    assert (w, h, len(ch)) == (W, H, 25)
    rec = records(r)
    assert (ch["A"] > 0).any() and np.isinf(ch["Z"]).sum() == (rec["hits"] == 0).sum() and (ch["id0"] == rec["id"][..., 0]).all()
    assert ch["R"].max() > 0 and ch["denoised.G"].max() > 0 and (ch["normal.Z"] != 0).any() and (ch["albedo.B"] > 0).any()
    same(r.exr(layers=abi.EXR_ALL, beauty="denoised_mean"), numpy_file(r, abi.EXR_ALL, "denoised_mean"), "beauty from the denoised mean")
    # rene_write_exr writes the same file
    p = api._exr_params(abi.EXR_ALL, "radiance")
    api._check(api.lib().rene_write_exr(r._h, C.byref(p), str(tmp_path / "w.exr").encode()))
    assert (tmp_path / "w.exr").read_bytes() == got
    assert api.lib().rene_write_exr(r._h, C.byref(p), str(tmp_path / "no" / "such" / "w.exr").encode()) == -6


@pytest.mark.parametrize("mask", [abi.EXR_BEAUTY, abi.EXR_DEFAULT, abi.EXR_BEAUTY | abi.EXR_DEPTH, GEOMETRY, abi.EXR_DENOISED | abi.EXR_IDS | abi.EXR_NORMAL])
def test_layer_masks_on_the_odd_width(job, mask):
    same(job.exr(layers=mask), numpy_file(job, mask), hex(mask))


def test_even_width():
    with api.Renderer(scenes.cornell_box(64, 33)) as r:
        r.render(0, FRAMES)
        r.gbuffer(GB_FIRST, GB_FRAMES)
        for mask in (abi.EXR_BEAUTY, abi.EXR_BEAUTY | abi.EXR_DEPTH):
            same(r.exr(layers=mask), numpy_file(r, mask), hex(mask))
        r.resolve_robust()
        same(r.exr(layers=abi.EXR_BEAUTY | abi.EXR_ALPHA, beauty="robust"), numpy_file(r, abi.EXR_BEAUTY | abi.EXR_ALPHA, "robust"), "robust beauty")
        # rene_reset leaves the geometry records alone: the layers that read them are still there, beside the means of a context without frames
        depth = er.parse(r.exr(layers=abi.EXR_BEAUTY | abi.EXR_DEPTH))[2]["Z"]
        r.reset()
        assert code(lambda: r.exr(beauty="robust")) == -1
        after = er.parse(r.exr(layers=abi.EXR_BEAUTY | abi.EXR_DEPTH))[2]
        assert after["Z"].tobytes() == depth.tobytes() and not after["R"].any()


@pytest.mark.parametrize("n", [1, 3])
def test_crafted_radiance_at_the_edges_of_the_half_format(n):
    w, h = 33, 2
    with np.errstate(all="ignore"):
        film = np.resize(np.concatenate([er.EDGE_VALUES, -er.EDGE_VALUES, er.EDGE_VALUES * np.float32(n)]), (h, w, 3)).astype(np.float32)
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.load_chains(cr.single_chain_load(film, 1.0), 0, n)
        mean = r.download_mean(0)
        flat = mean.reshape(-1)
        assert np.isnan(flat).any() and (np.abs(flat[np.isfinite(flat)]) > 65504).any() and (np.signbit(flat) & (flat == 0)).any()
        assert ((np.abs(flat) > 0) & (np.abs(flat) < 2.0 ** -14)).any(), "a mean in the range of the half subnormals"
        if n == 1:
            assert np.array_equal(np.nan_to_num(mean, nan=7.0), np.nan_to_num(film, nan=7.0))
        want = api.exr_header(w, h, abi.EXR_DEFAULT) + api.exr_body_host(w, h, abi.EXR_DEFAULT, beauty=mean, albedo=r.download_mean(2), normal=r.download_mean(1))
        got = r.exr()
        same(got, want, f"crafted, N = {n}")
        same(got, numpy_file(r, abi.EXR_DEFAULT), f"crafted against numpy, N = {n}")
        red = er.parse(got)[2]["R"]
        assert np.isfinite(red[~np.isnan(mean[..., 0])]).all() and np.isnan(red[np.isnan(mean[..., 0])]).all()


def test_adaptive_context_divides_every_tile_by_its_own_count():
    classes = ar.tile_classes(W, H)
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        ar.run_schedule(r, classes)
        assert sorted(np.unique(r.tile_frames())) == [0, 11, 19, 35]
        got = r.exr()
        same(got, numpy_file(r, abi.EXR_DEFAULT), "adaptive")
        ch = er.parse(got)[2]
        for (ty, tx), (rows, cols) in ar.tile_slices(W, H):
            if classes[ty, tx] == "A":  # N_t == 0: 0
                assert not any(ch[name][rows, cols].any() for name in ch), (ty, tx)
        assert (ch["R"] > 0).any() and (ch["albedo.R"] > 0).any()
        r.denoise_tiles()
        mask = abi.EXR_BEAUTY | abi.EXR_DENOISED
        same(r.exr(layers=mask, beauty="denoised_mean"), numpy_file(r, mask, "denoised_mean"), "adaptive, denoised tile by tile")


def test_three_tile_shards_fill_one_tensor():
    import torch
    s = scenes.cornell_box(W, H)
    mask = NO_DENOISED
    head, body, _ = api.exr_layout(W, H, mask)
    with api.Renderer(s) as whole:
        whole.render(0, FRAMES)
        whole.gbuffer(GB_FIRST, GB_FRAMES)
        want = np.frombuffer(whole.exr(layers=mask), np.uint8)[head:]
    tiles = np.arange(6).reshape(2, 3)
    owner = np.repeat(np.repeat(tiles, 32, axis=0), 32, axis=1)[:H, :W] % 3
    rs = [api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=3) for k in range(3)]
    try:
        t = torch.full((body,), 0xAB, dtype=torch.uint8, device="cuda:0")
        written = np.zeros(body, bool)
        for k, r in enumerate(rs):
            r.render(0, FRAMES)
            r.gbuffer(GB_FIRST, GB_FRAMES)
            alone = torch.full((body,), 0xAB, dtype=torch.uint8, device="cuda:0")
            got = r.exr_into(alone, layers=mask).cpu().numpy()
            own = er.owned_bytes(mask, owner == k)
            assert np.array_equal(got[own], want[own]), k
            assert (got[~own] == 0xAB).all(), k  # every byte it does not own is left as it was
            written |= own
            assert r.exr_into(t, layers=mask) is t
            assert code(lambda: r.exr(layers=abi.EXR_DENOISED)) == -4 and code(lambda: r.exr(beauty="denoised_mean")) == -4  # RENE_ERR_UNSUPPORTED, as rene_output_8bit
        assert written.all()
        assert np.array_equal(t.cpu().numpy(), want)
        lib_own = np.frombuffer(rs[1].exr(layers=mask), np.uint8)[head:]  # a shard's own buffer: its bytes, zero elsewhere
        own = er.owned_bytes(mask, owner == 1)
        assert np.array_equal(lib_own[own], want[own]) and not lib_own[~own].any()
    finally:
        for r in rs:
            r.close()


def test_the_call_changes_nothing_it_reads():
    s = scenes.cornell_box(W, H)
    counters = lambda r: {k: v for k, v in r.stats().as_dict().items() if "ms" not in k and k != "sclk_mhz"}
    with api.Renderer(s) as a, api.Renderer(s) as b:
        a.render(0, FRAMES)
        a.gbuffer(GB_FIRST, GB_FRAMES)
        a.denoise()
        before = (a.download_denoised(abi.DENOISED_RADIANCE), a.download_denoised(abi.DENOISED_MEAN), a.download_denoised(abi.DENOISED_VARIANCE), records(a))
        first = a.exr(layers=abi.EXR_ALL)
        after = (a.download_denoised(abi.DENOISED_RADIANCE), a.download_denoised(abi.DENOISED_MEAN), a.download_denoised(abi.DENOISED_VARIANCE), records(a))
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes()
        assert a.exr(layers=abi.EXR_ALL) == first and a.exr(layers=abi.EXR_ALL, beauty="denoised_mean") != first
        a.render(FRAMES, FRAMES)
        b.render(0, FRAMES)
        b.render(FRAMES, FRAMES)
        for l in range(3):
            assert a.download(l).tobytes() == b.download(l).tobytes(), l
        assert counters(a) == counters(b)


def test_destinations_and_refusals():
    import torch
    L = api.lib()
    mask = abi.EXR_DEFAULT
    need = api.exr_layout(W, H, mask)[1]
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        assert code(r.exr_buffer) == -1
        r.render(0, FRAMES)
        want = r.exr()
        p = api.exr_params_default()
        call = lambda p, ptr, n: L.rene_output_exr(r._h, C.byref(p), C.c_void_p(ptr), n)
        host = np.full(need, 0xAB, np.uint8)
        assert call(p, host.ctypes.data, host.nbytes) == -1 and L.rene_last_error()  # a host pointer never reaches a kernel
        assert (host == 0xAB).all()
        t = torch.full((need + 8,), 0xAB, dtype=torch.uint8, device="cuda:0")
        assert call(p, t.data_ptr(), need - 1) == -1 and b"dst_bytes" in L.rene_last_error()  # one byte short
        assert call(p, t.data_ptr() + 2, need) == -1 and b"aligned" in L.rene_last_error()    # an address = 2 (mod 4)
        for field, bad in (("struct_size", 12), ("layers", 0), ("layers", 256), ("beauty_source", abi.OUTPUT_DENOISED), ("beauty_source", 6), ("reserved", 1)):
            q = api.exr_params_default()
            setattr(q, field, bad)
            assert call(q, t.data_ptr(), need) == -1 and L.rene_last_error(), (field, bad)
        # a layer whose own call has not run: the geometry pass, the denoiser, the robust resolve
        for layers, beauty in ((abi.EXR_ALPHA, "radiance"), (abi.EXR_DEPTH | abi.EXR_BEAUTY, "radiance"), (abi.EXR_IDS, "radiance"), (abi.EXR_POSITION, "radiance"),
                               (abi.EXR_DENOISED, "radiance"), (abi.EXR_BEAUTY, "denoised_mean"), (abi.EXR_BEAUTY, "robust")):
            q = api._exr_params(layers, beauty)
            assert call(q, t.data_ptr(), t.numel()) == -1 and L.rene_last_error(), (layers, beauty)
        assert (t == 0xAB).all().item()  # nothing was launched on it
        for bad in (torch.zeros((need - 1,), dtype=torch.uint8, device="cuda:0"), torch.zeros((need,), device="cuda:0"),
                    torch.zeros((2 * need,), dtype=torch.uint8, device="cuda:0")[::2], torch.zeros((need,), dtype=torch.uint8)):
            with pytest.raises((TypeError, ValueError)):
                r.exr_into(bad)
        assert code(lambda: r.exr_into(t[2:need + 2])) == -1  # misaligned, refused by the library
        assert (t == 0xAB).all().item()
        assert r.exr_into(t[4:need + 4]) is not None and bytes(t[4:need + 4].cpu().numpy()) == want[-need:]  # the context is usable afterwards
        assert (t[:4] == 0xAB).all().item() and (t[need + 4:] == 0xAB).all().item()
        small = np.zeros(8, np.uint8)
        assert L.rene_download_exr(r._h, small.ctypes.data_as(C.c_void_p), small.nbytes) == -1
        assert r.exr() == want
        r.reset()
        assert code(r.exr_buffer) == -1
        assert not np.frombuffer(r.exr(), np.uint8)[-need:].reshape(H, -1)[:, 8:].any()  # no frames: N_t = 0 everywhere
    with api.Renderer(scenes.cornell_box(W, H), shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        r.render(0, 8)
        assert code(r.exr) == -4  # a frame shard holds a share of every pixel's frames


def test_command_line_writes_the_file(hip_lib, tmp_path):
    p = tmp_path / "scene.pbrt"
    p.write_text(loader.scene_to_pbrt(scenes.cornell_box(W, H)))
    run = subprocess.run([CLI, str(p), "--spp", "8", "--exr", "out.exr", "--exr-layers", "beauty,albedo,normal,depth", "--out", "x.exr"],
                         capture_output=True, text=True, cwd=tmp_path, env={**os.environ, "RENE_DEBUG": "1"})
    assert run.returncode == 0, run.stderr
    assert run.stderr.count("[rene] exr body ") == 1 and run.stderr.count("[rene] gbuffer ") == 1, run.stderr  # the device packed it, behind one geometry pass
    assert "INFO .exr output is not yet supported. Save as .png" in run.stderr and (tmp_path / "x.exr.png").exists() and not (tmp_path / "x.exr").exists()
    w, h, ch = er.parse((tmp_path / "out.exr").read_bytes())
    assert (w, h) == (W, H) and list(ch) == ["B", "G", "R", "Z", "albedo.B", "albedo.G", "albedo.R", "normal.X", "normal.Y", "normal.Z"]
    with api.Renderer(loader.load_pbrt(str(p))) as r:
        r.render(0, 8)
        mean = er.half(r.download_mean(0))
        for k, name in enumerate("RGB"):
            assert np.array_equal(ch[name].view(np.uint16), mean[..., k].view(np.uint16)), name
        assert np.array_equal(ch["normal.X"].view(np.uint16), er.half(r.download_mean(1))[..., 0].view(np.uint16))
        depth = er.gbuffer_planes(r.gbuffer(0, 8))["depth"]
        assert np.array_equal(ch["Z"].view(np.uint32), depth.view(np.uint32)) and ch["Z"].dtype == np.float32
    assert ch["R"].max() > 0 and np.isfinite(ch["Z"]).any()

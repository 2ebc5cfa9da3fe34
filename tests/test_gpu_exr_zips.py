"""GPU: the compressed OpenEXR output on the device (rene_exr_compress, rene_output_exr_compressed, include/rene_hip.h).  Everything here compares
BYTES with the host's rene_exr_compress_host, which tests/test_exr_zips_host.py holds to the specification: crafted bodies at every edge of the token
rule and of the kernels' segments, 1 MB rows, a rendered job with every layer read back by an independent reader, two tile shards that fill one
body, the files the library and the command line write, and the paths that must not change."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exr_reference as er
import exr_zips_reference as zr
from conftest import ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
W, H, FRAMES = 71, 45, 16  # odd W, ragged tiles
CASES = zr.cpu_cases() + zr.segment_cases()
IDS = [c[0] for c in CASES]


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
def ctx():
    """A context of a tiny Cornell film: rene_exr_compress takes any body, whatever the context's film."""
    with api.Renderer(scenes.cornell_box(16, 8)) as r:
        yield r


def device_tail(r, w, h, mask, body, compression="zips"):
    """The tail by the device into a tensor pre-filled with 0xA5 (nothing behind `written` may change), and by the device into the library's buffer."""
    import torch
    t_body = torch.frombuffer(bytearray(body), dtype=torch.uint8).to("cuda:0")
    bound = api.exr_tail_bound(w, h, mask)
    dst = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out, written = r.exr_compress(dst, w, h, mask, t_body, compression)
    assert out is dst and 16 * h <= written <= bound
    got = dst.cpu().numpy()
    assert (got[written:] == 0xA5).all(), "bytes behind `written` were written"
    own = r.exr_compress(None, w, h, mask, t_body, compression)
    assert r.download_exr_tail() == own and api._result_buffer(r, api.lib().rene_exr_tail_buffer)[1] == len(own)
    same(own, got[:written].tobytes(), "the library-owned tail against the caller-owned")
    assert bytes(t_body.cpu().numpy()) == bytes(body)  # the body is read, not written
    return got[:written].tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_crafted_bodies_equal_the_host(ctx, case):
    name, w, h, mask, body = case
    want = api.exr_compress_host(w, h, mask, body, "zips")
    same(device_tail(ctx, w, h, mask, body), want, name)
    if name.startswith("rows of "):
        assert zr.read(api.exr_attributes(w, h, mask, "zips") + want)[4] == [False] * 7 + [True]
    if name == "intervals at every segment edge":
        stored = zr.read(api.exr_attributes(w, h, mask, "zips") + want)[4]
        assert stored.count(True) == 1  # every row but the literals-only one is compressed: the encode kernel wrote their bits


def test_one_megabyte_rows(ctx):
    """16384 x 2 with every layer: rows of 1081344 bytes, 264 segments.  Row 0 is constant in every channel -- over 4000 maximal matches and
    Adler sums that need 64 bits -- row 1 is random and stored raw."""
    w, h, mask = 16384, 2, abi.EXR_ALL
    n = w * 66
    rng = np.random.default_rng(5)
    row0 = np.concatenate([np.resize(rng.integers(1, 256, 2 if t == "half" else 4, dtype=np.uint8), w * (2 if t == "half" else 4)) for _, _, t in abi.EXR_CHANNELS])
    body = zr.body_of([row0.tobytes(), rng.integers(0, 256, n, dtype=np.uint8).tobytes()])
    want = api.exr_compress_host(w, h, mask, body, "zips")
    sizes = [np.frombuffer(want, "<i4", 1, 16 + 4)[0]]
    sizes.append(np.frombuffer(want, "<i4", 1, 16 + 8 + sizes[0] + 4)[0])
    assert sizes[1] == n and 4000 * 13 // 8 < sizes[0] < n // 50  # 13 bits per full match
    d = zr.preprocess(row0.tobytes()).astype(np.int64)
    assert int(((n - np.arange(n)) * d).sum()) > 2 ** 40  # the second Adler sum before its reduction
    same(device_tail(ctx, w, h, mask, body), want, "1 MB rows")


def test_no_compression_and_refusals(ctx):
    import torch
    L = api.lib()
    name, w, h, mask, body = CASES[0]
    same(device_tail(ctx, w, h, mask, body, "none"), api.exr_header(w, h, mask)[-8 * h:] + body, "NONE: the present table and body")
    t_body = torch.frombuffer(bytearray(body), dtype=torch.uint8).to("cuda:0")
    bound = api.exr_tail_bound(w, h, mask)
    dst = torch.full((bound + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    written = C.c_size_t(77)
    call = lambda comp, b, nb, d, nd: L.rene_exr_compress(ctx._h, w, h, mask, comp, C.c_void_p(b), nb, C.c_void_p(d), nd, C.byref(written))
    for comp in (1, 3, 4, 255):
        assert call(comp, t_body.data_ptr(), len(body), dst.data_ptr(), bound) == -1 and b"compression" in L.rene_last_error()
    assert call(2, t_body.data_ptr(), len(body) - 1, dst.data_ptr(), bound) == -1 and b"body_bytes" in L.rene_last_error()
    assert call(2, t_body.data_ptr(), len(body), dst.data_ptr(), bound - 1) == -1 and b"dst_bytes" in L.rene_last_error()
    assert call(2, t_body.data_ptr(), len(body), dst.data_ptr() + 4, bound) == -1 and b"aligned" in L.rene_last_error()
    assert call(2, None, len(body), dst.data_ptr(), bound) == -1
    host = np.frombuffer(body, np.uint8).copy()
    assert call(2, host.ctypes.data, len(body), dst.data_ptr(), bound) == -1  # a host pointer never reaches a kernel
    host_dst = np.full(bound, 0xA5, np.uint8)
    assert call(2, t_body.data_ptr(), len(body), host_dst.ctypes.data, bound) == -1 and (host_dst == 0xA5).all()
    both = torch.zeros((len(body) + bound + 8,), dtype=torch.uint8, device="cuda:0")
    assert call(2, both.data_ptr(), len(body), both.data_ptr() + 8, bound) == -1 and b"overlaps" in L.rene_last_error()
    assert L.rene_exr_compress(ctx._h, w, h, mask, 2, C.c_void_p(t_body.data_ptr()), len(body), C.c_void_p(dst.data_ptr()), bound, None) == -1
    own = api._result_buffer(ctx, L.rene_exr_tail_buffer)[0]  # the library's tail buffer as the body of a call that overwrites it
    assert L.rene_exr_compress(ctx._h, w, h, mask, 2, C.c_void_p(own), len(body), None, 0, C.byref(written)) == -1 and b"tail buffer" in L.rene_last_error()
    assert written.value == 77 and (dst == 0xA5).all().item()  # nothing was launched
    with pytest.raises((TypeError, ValueError)):
        ctx.exr_compress(None, w, h, mask, t_body.cpu())


@pytest.fixture(scope="module")
def job():
    """Cornell 71 x 45: 16 frames, the geometry pass over them, denoised."""
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.render(0, FRAMES)
        r.gbuffer(0, FRAMES)
        r.denoise()
        yield r


def test_rendered_job_with_every_layer(job, tmp_path):
    import torch
    r, mask = job, abi.EXR_ALL
    plain = r.exr(layers=mask)
    head = api.exr_layout(W, H, mask)[0]
    body = plain[head:]
    attrs = api.exr_attributes(W, H, mask, "zips")
    want = api.exr_compress_host(W, H, mask, body, "zips")
    got = r.exr(layers=mask, compression="zips")
    same(got, attrs + want, "the file of a rendered job")
    rw, rh, chans, compression, stored = zr.read(got)
    pw, ph, ref = er.parse(plain)
    assert (rw, rh, compression) == (W, H, 2) and list(chans) == list(ref) and len(chans) == 25
    for name in ref:
        assert np.array_equal(chans[name].view(np.uint8), ref[name].view(np.uint8)), name
    assert not all(stored), "at least one row is compressed"
    assert len(got) < len(plain)
    # into a tensor of the caller's
    bound = api.exr_tail_bound(W, H, mask)
    t = torch.full((bound,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out, written = r.exr_into(t, layers=mask, compression="zips")
    assert out is t and written == len(want)
    host = t.cpu().numpy()
    same(host[:written].tobytes(), want, "exr_into, compressed")
    assert (host[written:] == 0xA5).all()
    # no compression through the new calls: the old bytes; and the old call is what it was
    out, written = r.exr_into(t, layers=mask, compression=abi.EXR_COMPRESSION_NONE)
    assert written == bound and api.exr_attributes(W, H, mask, "none") + t.cpu().numpy().tobytes() == plain
    assert r.exr(layers=mask) == plain
    # the files
    p = api._exr_params(mask, "radiance")
    api._check(api.lib().rene_write_exr_compressed(r._h, C.byref(p), 2, str(tmp_path / "w.exr").encode()))
    assert (tmp_path / "w.exr").read_bytes() == got
    assert r.exr(path=str(tmp_path / "p.exr"), layers=mask, compression="zips") == got and (tmp_path / "p.exr").read_bytes() == got
    api._check(api.lib().rene_write_exr_compressed(r._h, C.byref(p), 0, str(tmp_path / "n.exr").encode()))
    assert (tmp_path / "n.exr").read_bytes() == plain
    assert api.lib().rene_write_exr_compressed(r._h, C.byref(p), 2, str(tmp_path / "no" / "such" / "w.exr").encode()) == -6
    # rene_output_exr's refusals
    written = C.c_size_t()
    for field, bad in (("struct_size", 12), ("layers", 0), ("layers", 256), ("beauty_source", 6), ("reserved", 1)):
        q = api.exr_params_default()
        setattr(q, field, bad)
        assert api.lib().rene_output_exr_compressed(r._h, C.byref(q), 2, None, 0, C.byref(written)) == -1, (field, bad)
    assert api.lib().rene_output_exr_compressed(r._h, C.byref(p), 3, None, 0, C.byref(written)) == -1
    assert api.lib().rene_output_exr_compressed(r._h, C.byref(p), 2, C.c_void_p(t.data_ptr()), bound - 1, C.byref(written)) == -1
    r.reset()
    assert code(r.download_exr_tail) == -1  # invalidated like the other results of the frames
    r.render(0, FRAMES)
    r.denoise()


def test_two_tile_shards_fill_one_body():
    import torch
    s = scenes.cornell_box(W, H)
    mask = abi.EXR_ALL & ~abi.EXR_DENOISED
    head, body, _ = api.exr_layout(W, H, mask)
    with api.Renderer(s) as whole:
        whole.render(0, FRAMES)
        whole.gbuffer(0, FRAMES)
        want = whole.exr(layers=mask, compression="zips")
    rs = [api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=2) for k in range(2)]
    try:
        t = torch.full((body,), 0xAB, dtype=torch.uint8, device="cuda:0")
        for r in rs:
            r.render(0, FRAMES)
            r.gbuffer(0, FRAMES)
            r.exr_into(t, layers=mask)
            assert code(lambda: r.exr(layers=mask, compression="zips")) == -4  # RENE_ERR_UNSUPPORTED: a row spans tiles of several shards
        tail = rs[0].exr_compress(None, W, H, mask, t)
        same(api.exr_attributes(W, H, mask, "zips") + tail, want, "two shards' body, compressed by one")
    finally:
        for r in rs:
            r.close()


def test_command_line_writes_the_same_file(hip_lib, tmp_path):
    from test_images import load
    p = tmp_path / "scene.pbrt"
    p.write_text(loader.scene_to_pbrt(scenes.cornell_box(W, H)))
    layers = "beauty,albedo,normal,alpha,depth"
    run = subprocess.run([CLI, str(p), "--spp", "8", "--exr", "out.exr", "--exr-layers", layers, "--exr-compression", "zips"],
                         capture_output=True, text=True, cwd=tmp_path, env={**os.environ, "RENE_DEBUG": "1"})
    assert run.returncode == 0, run.stderr
    assert run.stderr.count("[rene] exr body ") == 1 and run.stderr.count("[rene] exr zips ") == 1, run.stderr
    got = (tmp_path / "out.exr").read_bytes()
    mask = api.exr_mask(layers.split(","))
    with api.Renderer(loader.load_pbrt(str(p))) as r:
        r.render(0, 8)
        r.gbuffer(0, 8)
        params = api._exr_params(mask, "radiance")
        api._check(api.lib().rene_write_exr_compressed(r._h, C.byref(params), 2, str(tmp_path / "lib.exr").encode()))
        plain = r.exr(layers=mask)
    assert (tmp_path / "lib.exr").read_bytes() == got  # the two files are equal
    w, h, chans, compression, stored = zr.read(got)
    ref = er.parse(plain)[2]
    assert (w, h, compression) == (W, H, 2) and all(np.array_equal(chans[n].view(np.uint8), ref[n].view(np.uint8)) for n in ref)
    rgba = load(tmp_path, "out.exr").reshape(H, W, 4)  # the library's own loader reads it
    for k, name in enumerate("RGBA"):
        assert np.array_equal(rgba[..., k], ref[name].astype(np.float32)), name
    # without the option: the uncompressed file, as before
    run = subprocess.run([CLI, str(p), "--spp", "8", "--exr", "plain.exr", "--exr-layers", layers], capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 0 and (tmp_path / "plain.exr").read_bytes() == plain

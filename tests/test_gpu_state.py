"""GPU: the checkpoint of a render job (rene_save_state / rene_restore_state and their file forms, include/rene_hip.h; kernels_state.hip).
A job that is saved, restored into a fresh context and rendered on is bit for bit the job that was never interrupted -- in every layer, on
every kernel family, under adaptive sampling and on any tile-shard layout; the bits of crafted chains survive the round trip; the chunking of
the pipeline changes no byte; what does not fit a context is refused before anything is written.  tests/state_reference.py parses the parts
from the format text alone."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_reference as ar
import chain_reference as cr
import state_reference as sr
from conftest import GOLDEN, ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
INVALID_ARGUMENT, UNSUPPORTED = -1, -4
W, H = 100, 70  # 4 x 3 tiles, ragged both ways

SCENES = {"dragon": (lambda: scenes.dragon_class(160, 90, 40, 44), 0), "teapot": (lambda: scenes.teapot_class(128, 72, 40, 44), 0),
          "fog": (lambda: scenes.dragon_fog(128, 72, 40, 44), 0), "cornell": (lambda: scenes.cornell_box(96, 64), 0),
          "veach": (lambda: scenes.veach_mis(96, 54), 0), "cornell-wavefront": (lambda: scenes.cornell_box(96, 64), abi.FLAG_WAVEFRONT),
          "dragon-no-restart": (lambda: scenes.dragon_class(160, 90, 40, 44), abi.FLAG_NO_RESTART)}


def refused(call, code, *words):
    with pytest.raises(api.ReneError) as e:
        call()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def image(r):
    """everything a context hands out of its accumulation state"""
    return [r.download(k) for k in range(3)] + [r.download_mean(0), r.tile_frames()]


def same_images(got, want, label):
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (label, i, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


@pytest.mark.parametrize("name, first", [(n, 0) for n in SCENES] + [("cornell", 100000), ("dragon", 100000)])
def test_resume_is_exact(hip_lib, name, first):
    """A: render(F, 19), save.  B, fresh: restore, render(F + 19, 16).  C: render(F, 35).  B == C in every layer, the means, the tiles' frame
    counts and the counts of frames and paths."""
    make, flags = SCENES[name]
    s = make()
    with api.Renderer(s, flags=flags) as a:
        a.render(first, 19)
        blob = a.save_state()
    api.state_verify(blob)
    info = api.state_info(blob)
    assert (info.frame_base, info.n_frames, info.loaded, info.frames_contiguous) == (first, 19, 0, 1)
    assert list(info.chain_frames) == sr.chain_frames(first, 19) and tuple(info.fingerprint) == api.scene_fingerprint(s)
    with api.Renderer(s, flags=flags) as b:
        b.restore_state(blob)
        assert b.stats().frames == 19 and b.stats().launches == 0  # launches count what this context itself does
        b.render(first + 19, 16)
        got, sb = image(b), b.stats()
    with api.Renderer(s, flags=flags) as c:
        c.render(first, 35)
        want, sc = image(c), c.stats()
    same_images(got, want, name)
    assert (sb.frames, sb.paths) == (sc.frames, sc.paths) == (35, 35 * s.film.xresolution * s.film.yresolution)


def crafted_film():
    film = cr.edge_chains(H, W, seed=5)[0].copy()  # NaN, infinities, overflow, ties among its classes
    bits = film.view(np.uint32)
    special = [0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000]  # NaN payloads, +-inf, -0.0, denormals
    rng = np.random.default_rng(9)
    for i, v in enumerate(special * 40):
        bits[rng.integers(8), rng.integers(3), rng.integers(H), rng.integers(W), rng.integers(3)] = v
    bits[:, :, H - 1, W - 1, :] = special[0]  # ... and in the corner of the ragged corner tile
    return film


def test_the_bits_survive(hip_lib):
    film = crafted_film()
    s = scenes.cornell_box(W, H)
    halves = abi.FEATURE_HALF_A | abi.FEATURE_HALF_B
    with api.Renderer(s) as a:
        a.load_chains(film, first_frame=3, n_frames=19)
        blob = a.save_state()
        want = [a.download(k) for k in range(3)] + [a.features(halves)]
    api.state_verify(blob)
    assert api.state_info(blob).loaded == 1
    assert np.array_equal(sr.chains_of(blob, W, H), film.view(np.uint32))  # per pixel, as uint32
    _, table, payload = sr.parse(blob)
    assert [sr.checksum_fast(p) for p in payload] == list(zip(table["c0"].tolist(), table["c1"].tolist()))
    with api.Renderer(s) as b:
        b.restore_state(blob)
        got = [b.download(k) for k in range(3)] + [b.features(halves)]
        same_images(got, want, "crafted")
        refused(lambda: b.render(22, 1), UNSUPPORTED, "rene_load_chains")  # `loaded` travelled
        again = b.save_state()
    assert np.array_equal(again, blob)


def test_adaptive_job_resumes(hip_lib):
    s = scenes.cornell_box(W, H)
    ty, tx = 3, 4
    first_off = np.ones((ty, tx), np.uint8)
    first_off[1, 2] = 0          # never renders: N_t = 0
    second_off = first_off.copy()
    second_off[0, 0] = second_off[2, 3] = second_off[1, 1] = 0
    third_off = second_off.copy()
    third_off[0, 3] = 0
    with api.Renderer(s) as a:
        a.set_active_tiles(first_off)
        a.render(0, 8)
        a.set_active_tiles(second_off)
        a.render(8, 8)
        blob = a.save_state()
        with api.Renderer(s) as b:
            b.restore_state(blob)
            tf = a.tile_frames()
            assert np.array_equal(b.tile_frames(), tf) and tf[1, 2] == 0 and tf[0, 0] == 8 and tf[0, 1] == 16
            t = api.state_tiles(blob)
            assert t["n_frames"].tolist() == tf.reshape(-1).tolist() and t["flags"].tolist() == second_off.reshape(-1).tolist()
            same_images(image(b), image(a), "restored")
            refused(lambda: b.set_active_tiles(first_off), INVALID_ARGUMENT, "cannot be set active again")
            for r in (a, b):  # shrinking further is accepted
                r.set_active_tiles(third_off)
                r.render(16, 8)
            same_images(image(b), image(a), "continued")
            assert np.array_equal(b.tile_frames(), np.where(third_off, 24, tf))
            assert (b.stats().frames, b.stats().paths) == (a.stats().frames, a.stats().paths)


def test_any_shard_layout(hip_lib):
    import torch
    s = scenes.cornell_box(W, H)
    tiles = np.arange(12).reshape(3, 4)
    with api.Renderer(s) as u:
        u.render(0, 19)
        part = u.save_state()
        u.render(19, 8)
        want, want_rgb = [u.download(k) for k in range(3)], u.rgb8()
    shards = [api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=2) for k in range(2)]
    try:
        t = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        for k, r in enumerate(shards):  # one unsharded part into two tile shards
            r.restore_state(part)
            r.render(19, 8)
            r.rgb8_into(t)
            for layer in range(3):
                got = r.download(layer)
                for (y, x), (rows, cols) in ar.tile_slices(W, H):
                    if tiles[y, x] % 2 == k:
                        assert np.array_equal(got[rows, cols], want[layer][rows, cols]), (k, layer, y, x)
        assert np.array_equal(t.cpu().numpy(), want_rgb)
        p0, p1 = (r.save_state() for r in shards)  # ... and the reverse: two shards' parts into one context
        assert api.state_tiles(p0)["tile"].tolist() == list(range(0, 12, 2)) and p0.size == api.state_bytes(W, H, 0, 2)
    finally:
        for r in shards:
            r.close()
    with api.Renderer(s) as one:
        refused(lambda: one.restore_state(p0), INVALID_ARGUMENT, "tile 1", "missing")
        assert one.stats().frames == 0 and not one.download(0).any()
        one.restore_state(p1, p0)  # (in any order)
        assert one.stats().frames == 27
        for layer in range(3):
            assert np.array_equal(one.download(layer), want[layer]), layer
        refused(lambda: one.restore_state(p0, p1), INVALID_ARGUMENT, "already holds frames")
    with api.Renderer(s) as one:
        refused(lambda: one.restore_state(p0, p1, p0), INVALID_ARGUMENT, "tile 0", "part 0", "part 2")


def test_chunking_changes_nothing(hip_lib, tmp_path):
    s = scenes.cornell_box(W, H)
    with api.Renderer(s) as a:
        a.render(0, 11)
        blobs = {c: a.save_state(chunk_tiles=c).copy() for c in (1, 2, 5, None)}
        a.save_state_file(tmp_path / "state.bin", chunk_tiles=2)
        want = image(a)
    for c in (1, 2, 5):
        assert np.array_equal(blobs[c], blobs[None]), c
    assert (tmp_path / "state.bin").read_bytes() == blobs[None].tobytes() and not (tmp_path / "state.bin.tmp").exists()
    for c in (1, 2, None):
        with api.Renderer(s) as b:
            b.restore_state(blobs[None], chunk_tiles=c)
            same_images(image(b), want, c)
    with api.Renderer(s) as b:
        b.restore_state_files(tmp_path / "state.bin", chunk_tiles=1)
        same_images(image(b), want, "file")
        b.save_state_file(tmp_path / "again.bin")
    assert (tmp_path / "again.bin").read_bytes() == blobs[None].tobytes()
    with api.Renderer(s) as b:
        refused(lambda: b.restore_state_files(tmp_path / "absent.bin"), -6, "cannot open")
        (tmp_path / "short.bin").write_bytes(blobs[None].tobytes()[:-5])
        refused(lambda: b.restore_state_files(tmp_path / "short.bin"), INVALID_ARGUMENT, "truncated")
        refused(lambda: b.save_state(), INVALID_ARGUMENT, "no frames")


def test_refusals_come_before_any_write(hip_lib):
    s = scenes.cornell_box(W, H)
    with api.Renderer(s) as a:
        a.render(0, 9)
        blob = a.save_state()
        before = image(a)
        refused(lambda: a.restore_state(blob), INVALID_ARGUMENT, "already holds frames")  # a context that holds frames
        same_images(image(a), before, "holds frames")

    def untouched(r, code, *words):
        zero = [r.download(k) for k in range(3)]
        refused(lambda: r.restore_state(blob), code, *words)
        same_images([r.download(k) for k in range(3)], zero, words)
        assert r.stats().frames == 0

    with api.Renderer(s, seed=7) as r:
        untouched(r, INVALID_ARGUMENT, "seed")
    with api.Renderer(scenes.cornell_box(W, H + 1)) as r:
        untouched(r, INVALID_ARGUMENT, "film")
    with api.Renderer(scenes.veach_mis(W, H)) as r:
        untouched(r, INVALID_ARGUMENT, "another scene")
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        untouched(r, UNSUPPORTED, "frame shard")
        r.render(0, 8)
        refused(lambda: r.save_state(), UNSUPPORTED, "frame shard")
    with api.Renderer(s) as r:  # an exchanged context
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 9)
        r.gather_tiles(0)
        ex = r.download(0)
        refused(lambda: r.save_state(), UNSUPPORTED, "rene_gather_tiles")
        refused(lambda: r.restore_state(blob), UNSUPPORTED, "rene_gather_tiles")
        assert np.array_equal(r.download(0), ex)
    # a payload bit flipped after saving: found on the device, after the upload; the context is then as reset leaves it
    bad = blob.copy()
    bad[256 + 12 * 32 + 7 * 294912 + 123456] ^= 0x04
    with api.Renderer(s) as r:
        refused(lambda: r.restore_state(bad), INVALID_ARGUMENT, "checksum mismatch in tile 7")
        assert r.stats().frames == 0 and not r.download(0).any() and r.tile_frames().max() == 0
        r.restore_state(blob)  # ... and takes the good part
        same_images(image(r), before, "after the bad part")


def test_a_shard_whose_tiles_have_all_stopped(hip_lib):
    """Its part carries its own N (the largest N_t in the part) and the chain counts of that N; the library reads what it wrote, alone and
    beside the part of the shard that went on."""
    s = scenes.cornell_box(W, H)
    odd_off = (np.arange(12).reshape(3, 4) % 2 == 0).astype(np.uint8)  # the tiles of shard 1 of 2 stop
    with api.Renderer(s) as u:
        u.render(0, 8)
        u.set_active_tiles(odd_off)
        u.render(8, 8)
        want, su = image(u), u.stats()
    shards = [api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=2) for k in range(2)]
    try:
        for r in shards:
            r.render(0, 8)
        shards[1].set_active_tiles(np.zeros((3, 4), np.uint8))
        for r in shards:
            r.render(8, 8)  # (shard 1 launches nothing and counts nothing)
        p0, p1 = (r.save_state() for r in shards)
        tf1 = shards[1].tile_frames()
    finally:
        for r in shards:
            r.close()
    i0, i1 = api.state_info(p0), api.state_info(p1)
    assert (i0.n_frames, i1.n_frames) == (16, 8) and list(i1.chain_frames) == sr.chain_frames(0, 8) and list(i0.chain_frames) == sr.chain_frames(0, 16)
    api.state_verify(p1)
    assert api.state_tiles(p1)["flags"].tolist() == [0] * 6 and api.state_tiles(p1)["n_frames"].tolist() == [8] * 6
    with api.Renderer(s) as one:
        one.restore_state(p1, p0)
        same_images(image(one), want, "two parts of different N")
        assert (one.stats().frames, one.stats().paths) == (su.frames, su.paths) == (16, 8 * W * H + 8 * int(ar.tile_pixels(W, H)[odd_off != 0].sum()))
        again = one.save_state()
    assert api.state_info(again).n_frames == 16 and api.state_tiles(again)["flags"].tolist() == odd_off.reshape(-1).tolist()
    with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=2) as r:
        r.restore_state(p1)
        assert r.stats().frames == 8 and np.array_equal(r.tile_frames(), tf1)
        got = r.download(0)
        for (y, x), (rows, cols) in ar.tile_slices(W, H):
            if (y * 4 + x) % 2 == 1:
                assert np.array_equal(got[rows, cols], want[0][rows, cols]), (y, x)
        assert np.array_equal(r.save_state(), p1)


def test_cli_adaptive_job_resumes_with_stopped_tiles(hip_lib, tmp_path):
    """A --target-noise --adaptive job whose checkpoint falls on one of its own batch boundaries, with tiles that have stopped by then: resumed with
    the same options it writes the bytes of the uninterrupted job.  The target is put between the noise of two tiles at the first estimate, so that
    some tiles stop there and others go on; the quietest tile that goes on then needs no more than a batch, so the uninterrupted job's second
    batch ends at frame 32 as the cut job's does."""
    from PIL import Image
    scene = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    ls = loader.load_pbrt(scene)
    ls.desc.xresolution = ls.desc.yresolution = ls.xres = ls.yres = 80
    with api.Renderer(ls) as r:
        r.render(0, 16)
        r.estimate_noise()
        noise = np.sort(np.sqrt(api.tile_noise(r.noise_tiles())).reshape(-1))
    target = float(noise[3] + noise[4]) / 2
    print("tile noise at 16 frames:", noise.tolist(), "target", target)
    assert noise[3] < target < noise[4] <= 1.7 * target  # (ceil(16 (noise / target)^2) <= 48: half of what is missing is at most a batch)
    opts = ["--width", "80", "--height", "80", "--adaptive", "--target-noise", repr(target), "--batch", "16", "--dilate", "0"]

    def run(*args):
        p = subprocess.run([CLI, scene, *opts, *args], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        return p.stderr

    run("--spp", "32", "--checkpoint", "f.state", "--out", "cut.png")
    info, tiles = api.state_file_info(tmp_path / "f.state")
    assert info.n_frames == 32 and sorted(set(tiles["n_frames"].tolist())) == [16, 32] and tiles["flags"].tolist() == (tiles["n_frames"] == 32).astype(int).tolist()
    log = run("--spp", "64", "--resume", "f.state", "--out", "a.png", "--sample-map", "m_a.png")
    assert "32 frames restored" in log and f"{int(tiles['flags'].sum())} of 9 tiles active" in log
    run("--spp", "64", "--out", "b.png", "--sample-map", "m_b.png")
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert (tmp_path / "m_a.png").read_bytes() == (tmp_path / "m_b.png").read_bytes()
    assert len(np.unique(np.asarray(Image.open(tmp_path / "m_a.png")))) > 1  # tiles did stop: the sample map is not uniform


@pytest.mark.parametrize("extra", [[], ["--adaptive", "--target-noise", "0.05", "--batch", "4"]], ids=["plain", "adaptive"])
def test_cli_resume_writes_the_same_bytes(hip_lib, tmp_path, extra):
    scene = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    size = ["--width", "80", "--height", "80"]

    def run(*args):
        p = subprocess.run([CLI, scene, *size, *extra, *args], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 0, p.stderr
        return p.stderr

    maps = lambda n: ["--sample-map", f"m_{n}.png"] if extra else []
    run("--spp", "8", "--checkpoint", "f.state", "--out", "first.png")
    api.state_verify(np.fromfile(tmp_path / "f.state", np.uint8))
    assert api.state_info(np.fromfile(tmp_path / "f.state", np.uint8)).n_frames == 8
    log = run("--spp", "16", "--resume", "f.state", "--out", "a.png", *maps("a"))
    assert "8 frames restored" in log
    run("--spp", "16", "--out", "b.png", *maps("b"))
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert (tmp_path / "a.png").read_bytes() != (tmp_path / "first.png").read_bytes()
    if extra:
        assert (tmp_path / "m_a.png").read_bytes() == (tmp_path / "m_b.png").read_bytes()
    p = subprocess.run([CLI, scene, "--gpus", "2", "--resume", "f.state"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and "--gpus" in p.stderr

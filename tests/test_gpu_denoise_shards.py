"""GPU: the `atrous` denoiser on tile shards (rene_denoise_shard_prepare, rene_denoise_place_shard, rene_denoise_placed, rene_gather_denoise) --
prepare on the shards, filter on one.  Nothing in the filter's arithmetic changes, so every comparison here is bit for bit: with rene_denoise on an
unsharded context where the tiles are even, with rene_denoise_tiles where they are not (two kinds of invalid tiles included); the packed records
tile by tile against the shard-of-one buffer; the way through host memory against the way through device pointers; the contract (read-only,
deterministic, independent of the cut, refusing what it cannot do with the documented codes); and the communicator of one.

All shard contexts sit on device 0 in one process, as in the shard tests of the chain passes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import atrous_tiles_reference as at
from conftest import ROOT
from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")

TILE, SLOTS = 32, 1024
INVALID_ARGUMENT, UNSUPPORTED = -1, -4

EVEN = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12),  # 12 tiles, ragged on both edges, chains of 2 and 1 frames
    "fog": (lambda: scenes.cornell_fog(96, 64), 32),       # the volpath kernel family
}
UNEVEN = lambda: scenes.cornell_box(161, 130)  # 30 tiles under the five-class schedule: N_t = 0, 1, 11, 19, 35


def results(r):
    return (r.download_denoised(channels=4), r.download_denoised(abi.DENOISED_VARIANCE), r.download_denoised(abi.DENOISED_MEAN, channels=4))


def assert_same(got, want, label):
    for g, w, what in zip(got, want, ("radiance", "variance", "mean")):
        assert np.array_equal(g, w), (label, what)


def make_shards(make, count):
    """The tile shards of a job, in rank order; None where rene_create does not admit a shard (one that owns no tile)."""
    out = []
    try:
        for rank in range(count):
            out.append(api.Renderer(make(), shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=count))
    except api.ReneError:
        close(out)
        return None
    return out


def close(renderers):
    for r in renderers:
        r.close()


def code_of(call, *args, **kw):
    with pytest.raises(api.ReneError) as e:
        call(*args, **kw)
    assert str(e.value).split(": ", 1)[1].strip()  # a message
    return e.value.code, str(e.value)


_even = {}


def even_reference(name):
    """Computed once per case and left unchanged: rene_denoise on the unsharded job, its layers, and its packed buffer as a shard of one."""
    if name not in _even:
        make, n = EVEN[name]
        with api.Renderer(make()) as r:
            r.render(0, n)
            layers = [r.download(l) for l in range(3)]
            r.denoise()
            want = results(r)
            r.denoise_shard_prepare()
            _even[name] = {"want": want, "layers": layers, "packed": r.download_denoise_shard(), "size": (r.xres, r.yres)}
        assert want[0].any() and want[1].any() and not want[0][..., 3].any()
    return _even[name]


# ---- 1. even jobs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,count", [("cornell", 1), ("cornell", 2), ("cornell", 3), ("cornell", 5), ("cornell", 16), ("fog", 2), ("fog", 3)])
def test_even_shards_equal_denoise_bit_for_bit(name, count):
    make, n = EVEN[name]
    ref = even_reference(name)
    shards = make_shards(make, count)
    if shards is None:
        pytest.skip(f"rene_create does not admit a shard that owns no tile ({count} shards)")
    try:
        for r in shards:
            r.render(0, n)
            r.denoise_shard_prepare()
        root = shards[0]
        for r in shards:
            ptr, size = r.denoise_shard_buffer()
            assert size == api.denoise_shard_bytes(*ref["size"], shards.index(r), count)
            root.denoise_place_shard(ptr, size)
        root.denoise_placed()
        assert_same(results(root), ref["want"], (name, count))
        ptr, floats = root.denoised_buffer()
        assert ptr and floats == ref["want"][0].size
    finally:
        close(shards)


def test_a_placed_body_is_read_after_its_copy_has_landed():
    """A packed buffer given as a device pointer is copied into the root's staging before the place kernel reads it; at 1024 x 512 a shard's body is
    13 MB, and a kernel that is not ordered behind that copy finds the body placed before it (the other rank's records, or a third context's).  Three
    rounds on a third context, each equal to rene_denoise bit for bit."""
    make = lambda: scenes.cornell_box(1024, 512)
    shards = make_shards(make, 2)
    try:
        for r in shards:
            r.render(0, 12)
            r.denoise_shard_prepare()
        with api.Renderer(make()) as root:
            root.render(0, 12)
            root.denoise()
            want = results(root)
            for k in range(3):
                for r in shards:
                    root.denoise_place_shard(*r.denoise_shard_buffer())
                root.denoise_placed()
                assert_same(results(root), want, ("round", k))
    finally:
        close(shards)


def test_even_shards_with_every_pass_direct(monkeypatch):
    """RENE_DENOISE_STAGE_MAX=0: no pass stages its tile in LDS -- the reference is taken under the same setting."""
    monkeypatch.setenv("RENE_DENOISE_STAGE_MAX", "0")
    make, n = EVEN["cornell"]
    with api.Renderer(make()) as r:
        r.render(0, n)
        r.denoise()
        want = results(r)
    shards = make_shards(make, 3)
    try:
        for r in shards:
            r.render(0, n)
        assert_same(results(api.denoise_shards(shards)), want, "stage_max 0")
    finally:
        close(shards)


# ---- 2. uneven tiles -----------------------------------------------------------------------------------------------------------------------------
def test_uneven_shards_equal_denoise_tiles_bit_for_bit():
    with api.Renderer(UNEVEN()) as r:
        classes = at.tile_classes(r.xres, r.yres)
        at.run_schedule(r, classes)
        r.denoise_tiles()
        want, plain, plain_mean = results(r), r.download(0, channels=4), r.download_mean(0, channels=4)
        frames = at.per_pixel(at.class_frames(classes), r.yres, r.xres)
    shards = make_shards(UNEVEN, 3)
    try:
        for r in shards:
            at.run_schedule(r, classes)
        got = results(api.denoise_shards(shards))
        assert_same(got, want, "uneven")
        invalid = frames < 2
        assert invalid.any() and (frames == 1).any() and (frames == 0).any()
        assert np.array_equal(got[0][invalid][:, :3], plain[invalid][:, :3])  # the radiance hands out rene_download's bits there
        assert np.array_equal(got[2][invalid][:, :3], plain_mean[invalid][:, :3]) and got[2][frames == 1].any()  # ... and the mean rene_download_mean's
        assert not got[1][invalid].any() and not np.array_equal(got[0][~invalid][:, :3], plain[~invalid][:, :3])
    finally:
        close(shards)


# ---- 3. the packed records ---------------------------------------------------------------------------------------------------------------------------
def parse(buf, xres, yres):
    """(header, table, blocks [n_owned][53248] uint8) of a packed buffer, by the layout of include/rene_hip.h."""
    h = abi.DenoiseShardHeader.from_buffer_copy(buf[:64].tobytes())
    assert h.magic == abi.DENOISE_SHARD_MAGIC and h.header_bytes == 64 and (h.width, h.height) == (xres, yres)
    table = buf[64:64 + 8 * h.n_owned].view(abi.DENOISE_SHARD_TILE_DTYPE)
    off = 64 + (8 * h.n_owned + 15) // 16 * 16
    assert not buf[64 + 8 * h.n_owned:off].any() and len(buf) == off + h.n_owned * abi.DENOISE_SHARD_TILE_BYTES
    return h, table, buf[off:].reshape(h.n_owned, abi.DENOISE_SHARD_TILE_BYTES)


def slot_pixels():
    """(dx, dy) of slot 0 .. 1023 inside its tile: 8 x 8 sub-blocks, the order of the frame chains."""
    r = np.arange(SLOTS)
    sub, l = r >> 6, r & 63
    return (sub & 3) * 8 + (l & 7), (sub >> 2) * 8 + (l >> 3)


def test_packed_records_tile_by_tile():
    make, n = EVEN["cornell"]
    ref = even_reference("cornell")
    xres, yres = ref["size"]
    tiles_x = -(-xres // TILE)
    h1, table1, blocks1 = parse(ref["packed"], xres, yres)
    assert (h1.shard_rank, h1.shard_count, h1.n_owned) == (0, 1, 12) and len(ref["packed"]) == api.denoise_shard_bytes(xres, yres)
    assert h1.params.iterations == 5 and h1.params.struct_size == C.sizeof(abi.DenoiseParams)
    assert (table1["n_frames"] == n).all() and (table1["valid"] == 1).all()
    dx, dy = slot_pixels()
    shards = make_shards(make, 3)
    try:
        seen = 0
        for rank, r in enumerate(shards):
            r.render(0, n)
            r.denoise_shard_prepare()
            buf = r.download_denoise_shard()
            assert len(buf) == api.denoise_shard_bytes(xres, yres, rank, 3) == r.denoise_shard_buffer()[1]
            h, table, blocks = parse(buf, xres, yres)
            assert (h.shard_rank, h.shard_count, h.n_owned) == (rank, 3, 4)
            assert bytes(h.params) == bytes(h1.params)
            for k in range(h.n_owned):
                t = rank + 3 * k
                assert np.array_equal(blocks[k], blocks1[t]), t  # the same bytes as in the shard-of-one buffer
                assert tuple(table[k]) == tuple(table1[t])
                f = blocks[k].view(np.float32)
                rec, guides, var = f[:4096].reshape(SLOTS, 4), f[4096:12288].reshape(SLOTS, 2, 4), f[12288:]
                x, y = (t % tiles_x) * TILE + dx, (t // tiles_x) * TILE + dy
                outside = (x >= xres) | (y >= yres)
                assert not rec[outside].any() and not guides[outside].any() and not var[outside].any()  # ragged tiles: zero records
                inside = ~outside
                assert np.array_equal(var[inside], ref["want"][1][y[inside], x[inside]])  # the variance plane, slot by slot
                assert np.array_equal(rec[inside, 3], var[inside])
                assert (guides[inside, 1, 2] == 1).all() and (guides[inside, 1, 3] == n).all()  # valid, (float)N_t
                seen += int(outside.sum())
        assert seen == 12 * SLOTS - xres * yres
    finally:
        close(shards)


# ---- 4. through host memory --------------------------------------------------------------------------------------------------------------------------
def test_host_round_trip_equals_device_pointers():
    make, n = EVEN["cornell"]
    ref = even_reference("cornell")
    shards = make_shards(make, 3)
    try:
        for r in shards:
            r.render(0, n)
        assert_same(results(api.denoise_shards(shards, root=1, via="host")), ref["want"], "host")  # (any context of the film can be the root)
        assert_same(results(api.denoise_shards(shards, root=1, via="device")), ref["want"], "device")
        with api.Renderer(make()) as bare:  # a root without frames of its own
            for r in shards:
                bare.denoise_place_shard(r.download_denoise_shard())
            bare.denoise_placed()
            assert_same(results(bare), ref["want"], "bare root")
    finally:
        close(shards)


# ---- 5. the contract -----------------------------------------------------------------------------------------------------------------------------
def test_read_only_deterministic_and_independent_of_the_cut():
    make, n = EVEN["cornell"]
    ref = even_reference("cornell")
    shards = make_shards(make, 2)
    try:
        for r in shards:
            r.render(0, 5)  # the job in two calls
            r.render(5, n - 5)
        before = [[r.download(l) for l in range(3)] for r in shards]
        first = results(api.denoise_shards(shards))
        assert_same(first, ref["want"], "cut")
        packed = [r.download_denoise_shard() for r in shards]
        assert_same(results(api.denoise_shards(shards)), first, "again")
        for r, b, pk in zip(shards, before, packed):
            assert np.array_equal(r.download_denoise_shard(), pk)
            for l in range(3):
                assert np.array_equal(r.download(l), b[l]), l  # chains and image untouched
        total = sum(b[0] for b in before)
        assert np.array_equal(total, ref["layers"][0])
        for r in shards:
            r.render(n, 4)  # rendering on after the denoise ...
        fresh = make_shards(make, 2)
        try:
            for r, f in zip(shards, fresh):
                f.render(0, n)
                f.render(n, 4)
                for l in range(3):
                    assert np.array_equal(r.download(l), f.download(l)), l  # ... equals the uninterrupted job
        finally:
            close(fresh)
    finally:
        close(shards)


def test_placed_and_place_refuse_with_the_documented_code():
    make, n = EVEN["cornell"]
    ref = even_reference("cornell")
    shards = make_shards(make, 3)
    others = make_shards(make, 2)
    try:
        for r in shards + others[:1]:
            r.render(0, n)
            r.denoise_shard_prepare()
        root = shards[0]
        code, msg = code_of(root.denoise_placed)  # nothing placed
        assert code == INVALID_ARGUMENT
        root.denoise_place_shard(shards[0].denoise_shard_buffer())
        root.denoise_place_shard(shards[2].denoise_shard_buffer())
        code, msg = code_of(root.denoise_placed)  # a rank missing
        assert code == INVALID_ARGUMENT and "rank(s) 1 " in msg
        code_of(root.download_denoised)  # no result while a round is open
        ptr, size = shards[1].denoise_shard_buffer()
        assert code_of(root.denoise_place_shard, ptr, size - 16)[0] == INVALID_ARGUMENT  # a wrong size
        assert code_of(root.denoise_place_shard, ptr, 32)[0] == INVALID_ARGUMENT
        assert code_of(root.denoise_place_shard, np.zeros(size, np.uint8))[0] == INVALID_ARGUMENT  # no header at all
        crafted = shards[1].download_denoise_shard()
        crafted[20:24] = np.frombuffer(np.uint32(0xFFFFFFF0).tobytes(), np.uint8)  # a shard_count no film has tiles for
        code, msg = code_of(root.denoise_place_shard, crafted)
        assert code == INVALID_ARGUMENT and "shard_count" in msg
        code, msg = code_of(root.denoise_place_shard, others[0].denoise_shard_buffer())  # another shard count
        assert code == INVALID_ARGUMENT and "2 shards" in msg
        shards[1].denoise_shard_prepare(iterations=3)
        code, msg = code_of(root.denoise_place_shard, shards[1].denoise_shard_buffer())  # other params
        assert code == INVALID_ARGUMENT and "params" in msg
        with api.Renderer(scenes.cornell_box(64, 64)) as small:  # a header of another film
            small.render(0, n)
            small.denoise_shard_prepare()
            code, msg = code_of(root.denoise_place_shard, small.denoise_shard_buffer())
            assert code == INVALID_ARGUMENT and "64 x 64" in msg
        # every refusal left the round as it was: the missing rank, prepared with the round's params, completes it
        shards[1].denoise_shard_prepare()
        ptr, size = shards[1].denoise_shard_buffer()
        root.denoise_place_shard(np.uint64(ptr), np.int64(size))  # (a pointer held in a numpy integer is a pointer)
        root.denoise_place_shard(shards[2].denoise_shard_buffer())  # placing a rank again replaces it
        root.denoise_placed()
        assert_same(results(root), ref["want"], "after refusals")
        assert code_of(root.denoise_placed)[0] == INVALID_ARGUMENT  # the round is over
    finally:
        close(shards + others)


def test_prepare_refuses_with_the_documented_code():
    make, n = EVEN["cornell"]
    ref = even_reference("cornell")
    with api.Renderer(make(), shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as f:  # a frame shard
        f.render(0, n)
        assert code_of(f.denoise_shard_prepare)[0] == UNSUPPORTED
        assert code_of(f.denoise_shard_buffer)[0] == INVALID_ARGUMENT
    with api.Renderer(make(), shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=2) as r:
        r.render(0, 1)  # a job of one frame: no owned tile is valid
        assert code_of(r.denoise_shard_prepare)[0] == INVALID_ARGUMENT
        assert code_of(r.denoise_shard_prepare, iterations=9)[0] == INVALID_ARGUMENT
        r.render(1, n - 1)
        assert r.download(0).max() > 0  # the context is usable
        r.denoise_shard_prepare()
        # the calls that take one context keep refusing a shard: the trimmed ones as before, the plain one pointing to the new calls
        code, msg = code_of(r.denoise, robust=True)
        assert code == UNSUPPORTED and "plain filter is available" in msg
        assert code_of(r.denoise_tiles, robust=True)[0] == UNSUPPORTED
        for call in (r.denoise, r.denoise_tiles):
            code, msg = code_of(call)
            assert code == UNSUPPORTED and "rene_denoise_shard_prepare" in msg and "rene_denoise_placed" in msg
        r.reset()
        assert code_of(r.denoise_shard_buffer)[0] == INVALID_ARGUMENT  # the reset discards the packed buffer
    with api.Renderer(make()) as r:  # an exchanged context: prepare comes before the gather, and what it made stays usable after it
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, n)
        r.denoise_shard_prepare()
        r.gather_tiles(0)
        assert code_of(r.denoise_shard_prepare)[0] == UNSUPPORTED
        r.denoise_place_shard(r.denoise_shard_buffer())
        r.denoise_placed()
        assert_same(results(r), ref["want"], "prepared before the gather")
        assert np.array_equal(r.download(0), ref["layers"][0])


# ---- 6. the communicator of one ----------------------------------------------------------------------------------------------------------------------
def test_gather_denoise_on_a_communicator_of_one():
    make, n = EVEN["cornell"]
    with api.Renderer(make()) as r:
        r.render(0, n)
        r.denoise_tiles()
        want = results(r)
        code, msg = code_of(r.gather_denoise, 0)
        assert code == INVALID_ARGUMENT and "rene_comm_init" in msg
        r.comm_init(1, 0, api.comm_unique_id())
        assert code_of(r.gather_denoise, 0)[0] == INVALID_ARGUMENT  # no packed buffer yet
        r.denoise_shard_prepare()
        assert code_of(r.gather_denoise, 1)[0] == INVALID_ARGUMENT  # root out of range
        r.gather_denoise(0)
        r.denoise_placed()
        assert_same(results(r), want, "communicator of one")
        # a reset between the gather and the filter discards what the gather left: placing by hand then works as on any root
        r.denoise_shard_prepare()
        r.gather_denoise(0)
        r.reset()
        r.render(0, n)
        r.denoise_shard_prepare()
        r.denoise_place_shard(r.denoise_shard_buffer())
        r.denoise_placed()
        assert_same(results(r), want, "after a reset")


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_firefly_rejection_on_several_gpus():
    """`--denoiser atrous --gpus G` itself is still refused by rene-hip (tests/test_denoise_host.py pins that); with --reject-fireflies the refusal
    says that the trimmed filter is what tile shards are not offered."""
    r = subprocess.run([CLI, "--gpus", "2", "--denoiser", "atrous", "--reject-fireflies", "x.pbrt"], capture_output=True, text=True)
    assert r.returncode == 2 and "--reject-fireflies cannot be combined with --gpus 2" in r.stderr and "plain filter" in r.stderr, r.stderr

"""GPU: the pass layers as an OpenEXR file, packed on the device (rene_output_exr_passes, include/rene_hip.h).  On a Cornell box with two lamps and a
sun at 77 x 45 (partial tiles on both edges), 8 frames rendered and the four passes run over frames 0 .. 7 into the library's buffers, the file is
BYTE FOR BYTE the independent numpy writer's (tests/exr_passes_reference.py) from the downloaded records and download(0), for every layer and five
other masks, on the item loop and on the BVH.  Crafted records at 33 x 2 -- uploaded through the `sources` pointers, the radiance through
load_chains -- hold the device's square root, divisions and half rounding at their edges against rene_exr_passes_body_host; three tile shards fill
one body; the call leaves the records, the chains and the denoiser's buffers alone; INDIRECT is refused where the frames do not match."""
import ctypes as C

import numpy as np
import pytest

import chain_reference
import exr_passes_reference as pr
import gbuffer_reference as gr
import lights_scenes
from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

W, H, FRAMES = 77, 45, 8
ALL = abi.EXRP_ALL
NAMES = [None, "sun", "key light", None, "rim-2", None, None, "fill_7"]
# every layer, single layers, two groups of eight, a pair that shares a record
MASKS = [(ALL, 0), (abi.EXRP_AO, 0), (abi.EXRP_INDIRECT, 0), (abi.EXRP_LIGHTS, 0x0A), (abi.EXRP_BOUNCES | abi.EXRP_LENGTH, 0),
         (abi.EXRP_BENT | abi.EXRP_DIRECT | abi.EXRP_LIGHTS, 0x81)]


def same(got, want, label):
    assert len(got) == len(want), (label, len(got), len(want))
    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert bad.size == 0, (label, len(bad), bad[:8].tolist())


def code(fn, word=None):
    with pytest.raises(api.ReneError) as e:
        fn()
    message = str(e.value).split(": ", 1)[1].strip()
    assert message and (word is None or word in message), message
    return e.value.code


def run_passes(r, first=0, frames=FRAMES):
    """The four passes into the library's buffers; their records on the host."""
    return dict(occlusion=r.occlusion(first, frames), direct=r.direct(first, frames), bounces=r.bounces(first, frames), lights=r.lights(first, frames))


_jobs = {}


def job(flags):
    if flags not in _jobs:
        r = api.Renderer(lights_scenes.cornell(W, H), flags=flags)
        r.render(0, FRAMES)
        rec = run_passes(r)
        rec["beauty_sum"] = r.download(0)
        _jobs[flags] = (r, rec)
    return _jobs[flags]


@pytest.fixture(scope="module", autouse=True)
def _close_jobs():
    yield
    for r, _ in _jobs.values():
        r.close()
    _jobs.clear()


def upload(a):
    import torch
    return torch.frombuffer(bytearray(a.tobytes()), dtype=torch.uint8).to("cuda:0")


def test_the_job_has_what_the_cases_need():
    _, rec = job(0)
    sums = rec["lights"]["group"]["sum"]
    assert sum(bool((sums[..., g, :] != 0).any()) for g in range(8)) >= 3, "two lamps and a sun: three groups at least"
    assert (rec["direct"]["n"] == FRAMES).all() and (rec["occlusion"]["rays"] == 0).any() and (rec["occlusion"]["occluded"] > 0).any()
    assert (rec["bounces"]["bucket"]["sum"][..., 3, :] != 0).any()


@pytest.mark.parametrize("flags", [0, abi.FLAG_FORCE_BVH])
@pytest.mark.parametrize("mask,groups", MASKS)
def test_the_file_is_the_reference_writers(flags, mask, groups):
    import torch
    r, rec = job(flags)
    want = pr.file_bytes(W, H, mask, groups, NAMES, **rec)
    same(r.exr_passes(layers=mask, groups=groups, group_names=NAMES), want, ("the library's buffer", mask, groups))
    attr_bytes, body_bytes, bpp = api.exr_passes_layout(W, H, mask, groups, NAMES)
    assert r.exr_passes_buffer()[1] == body_bytes == H * (8 + W * bpp) and bpp == pr.bytes_per_pixel(mask, groups)
    t = torch.full((body_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert r.exr_passes_into(t, layers=mask, groups=groups) is t
    host = t.cpu().numpy()
    same(host[:body_bytes].tobytes(), want[attr_bytes + 8 * H:], ("a caller's tensor", mask, groups))
    assert (host[body_bytes:] == 0xA5).all(), "bytes behind the body were written"


def test_crafted_records_against_the_host_form():
    """33 x 2: bpp 130, and with `ao` alone 2 -- row 1 starts at an address = 2 (mod 4)."""
    w, h = 33, 2
    c = pr.crafted(w, h)
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.load_chains(chain_reference.single_chain_load(c["beauty_sum"], 1.0), 0, 8)
        beauty = r.download(0)
        with np.errstate(all="ignore"):  # the radiance sums carry the crafted edges
            assert np.isnan(beauty).any() and np.isposinf(beauty).any() and np.isneginf(beauty).any() and (beauty < api.direct_sum(c["direct"])).any()
        sources = {k: upload(c[k]) for k in ("occlusion", "direct", "bounces", "lights")}
        host = dict(c, beauty_sum=beauty)
        for mask, groups in [(ALL, 0), (abi.EXRP_AO, 0), (abi.EXRP_AO | abi.EXRP_BENT, 0), (abi.EXRP_LENGTH | abi.EXRP_LIGHTS, 0x41), (abi.EXRP_INDIRECT, 0)]:
            want = api.exr_passes_body_host(w, h, mask, groups, **host)
            got = r.exr_passes(layers=mask, groups=groups, sources=sources)
            same(got[-len(want):], want, ("crafted", mask, groups))
            same(want, pr.body(w, h, mask, groups, **host), ("the host form is the reference's", mask, groups))
        for k, t in sources.items():
            assert t.cpu().numpy().tobytes() == c[k].tobytes(), k  # read, not written
        # a source whose layers are not chosen is not read: a bad pointer there is not looked at
        p, keep = api._exr_passes_params("ao", None, None, {"occlusion": sources["occlusion"].data_ptr(), "lights": 24})
        assert api.lib().rene_output_exr_passes(r._h, C.byref(p), None, 0) == 0


def test_three_tile_shards_fill_one_body():
    import torch
    r0, rec = job(0)
    want = pr.body(W, H, ALL, 0, **rec)
    bpp = pr.bytes_per_pixel(ALL)
    t = torch.full((len(want),), 0xAB, dtype=torch.uint8, device="cuda:0")
    written = np.zeros(len(want), bool)
    scene = lights_scenes.cornell(W, H)
    for rank in range(3):
        with api.Renderer(scene, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            r.render(0, FRAMES)
            run_passes(r)
            assert r.exr_passes_into(t) is t
            assert code(lambda: r.exr_passes(), "shards") == -4
            written |= pr.owned_bytes(bpp, gr.owned_mask(W, H, rank, 3))
            host = t.cpu().numpy()
            assert (host[~written] == 0xAB).all(), ("a shard wrote outside its pixels and its rows' prefixes", rank)
            same(host[written].tobytes(), np.frombuffer(want, np.uint8)[written].tobytes(), ("the shard's bytes", rank))
            if rank == 1:  # a shard's own buffer: its tiles' bytes, zeros elsewhere
                p, keep = api._exr_passes_params(ALL, None, None)
                api._check(api.lib().rene_output_exr_passes(r._h, C.byref(p), None, 0))
                part = api._download_result(r, api.lib().rene_download_exr_passes, (len(want),), np.uint8)
                own = pr.owned_bytes(bpp, gr.owned_mask(W, H, 1, 3))
                assert (part[~own] == 0).all() and part[own].tobytes() == np.frombuffer(want, np.uint8)[own].tobytes()
    assert written.all()
    same(t.cpu().numpy().tobytes(), want, "three shards' body")
    # a compressed file from the shards' body goes through exr_compress_rows
    attrs = api.exr_passes_attributes(W, H, ALL, compression="zips")
    same(attrs + r0.exr_compress_rows(W * bpp, H, len(attrs), t), r0.exr_passes(compression="zips"), "the shards' body, compressed by one context")


def test_the_call_leaves_the_state_alone():
    scene = lights_scenes.cornell(W, H)
    with api.Renderer(scene) as a, api.Renderer(scene) as b:
        for r in (a, b):
            r.render(0, FRAMES)
        rec = run_passes(a)
        a.denoise()
        denoised = a.download_denoised(abi.DENOISED_RADIANCE, 4)
        layers = [a.download(l, 4) for l in range(3)]
        st = bytes(a.stats())
        a.exr_passes()
        a.exr_passes(layers=("ao", "lights"), groups=(1, 3), compression="zips")
        assert all(a.download(l, 4).tobytes() == x.tobytes() for l, x in enumerate(layers)) and bytes(a.stats()) == st
        assert a.download_denoised(abi.DENOISED_RADIANCE, 4).tobytes() == denoised.tobytes()
        for name, dtype in (("occlusion", abi.OCCLUSION_DTYPE), ("direct", abi.DIRECT_DTYPE), ("bounces", abi.BOUNCES_DTYPE), ("lights", abi.LIGHTS_DTYPE)):
            again = api._download_result(a, getattr(api.lib(), "rene_download_" + name), (H, W), np.dtype(dtype))
            assert again.tobytes() == rec[name].tobytes(), name
        for r in (a, b):  # render - pack - render against render - render
            r.render(FRAMES, FRAMES)
        assert all(a.download(l, 4).tobytes() == b.download(l, 4).tobytes() for l in range(3))


def test_indirect_needs_the_direct_results_frames():
    scene = lights_scenes.cornell(W, H)
    with api.Renderer(scene) as r:
        r.render(0, 8)
        r.direct(0, 4)
        assert code(lambda: r.exr_passes(layers="indirect"), "frames") == -1  # 8 frames rendered, a pass over 0 .. 3
        assert len(r.exr_passes(layers="direct")) > 0  # (the direct layer alone has no such contract)
        rec = r.direct(0, 8)
        want = api.indirect_mean(r.download(0), rec)
        got = r.exr_passes(layers="indirect")
        planes = {k: v for k, v in zip(("indirect.B", "indirect.G", "indirect.R"), (want[..., 2], want[..., 1], want[..., 0]))}
        body = b"".join(np.int32([y, 6 * W]).tobytes() + b"".join(pr.half_bits(planes[k][y]).tobytes() for k in sorted(planes)) for y in range(H))
        same(got[-len(body):], body, "accepted, and api.indirect_mean's halves")
        r.direct(1, 8)
        assert code(lambda: r.exr_passes(layers="indirect"), "start") == -1  # the same count from another first frame
        r.reset()
        r.render(1, 8)
        assert len(r.exr_passes(layers="indirect")) == len(got)
    with api.Renderer(lights_scenes.cornell(100, 70)) as r:  # an adaptive context with uneven N_t
        r.render(0, 8)
        r.set_active_tiles(np.indices((3, 4)).sum(0) % 2)
        r.render(8, 8)
        for n in (8, 16):
            r.direct(0, n)
            assert code(lambda: r.exr_passes(layers=("direct", "indirect")), "frames") == -1
        assert len(r.exr_passes(layers="direct")) > 0


def test_refusals_before_anything_is_launched():
    import torch
    r, rec = job(0)
    need = api.exr_passes_layout(W, H, ALL)[1]
    t = torch.full((need + 8,), 0xAB, dtype=torch.uint8, device="cuda:0")
    L = api.lib()

    def call(dst, n, **fields):
        p, keep = api._exr_passes_params(fields.pop("layers", ALL), fields.pop("groups", None), fields.pop("group_names", None), fields.pop("sources", None))
        for k, v in fields.items():
            setattr(p, k, v)
        return L.rene_output_exr_passes(r._h, C.byref(p), dst, n), L.rene_last_error()

    assert call(C.c_void_p(t.data_ptr()), need - 1)[0] == -1 and b"dst_bytes" in L.rene_last_error()
    assert call(C.c_void_p(t.data_ptr() + 2), need)[0] == -1 and b"aligned" in L.rene_last_error()
    host = np.full(need, 0xAB, np.uint8)
    assert call(host.ctypes.data_as(C.c_void_p), need)[0] == -1 and (host == 0xAB).all()
    assert (t == 0xAB).all().item(), "a refused call wrote"
    for fields in (dict(struct_size=8), dict(layers=0), dict(layers=128), dict(layers=abi.EXRP_AO, groups=1), dict(groups=256), dict(reserved=1),
                   dict(group_names=['a"b'] + [None] * 7), dict(group_names=[""] + [None] * 7), dict(group_names=["x" * 25] + [None] * 7)):
        assert call(None, 0, **fields)[0] == -1, fields
    assert L.rene_output_exr_passes(None, None, None, 0) == -1 and L.rene_output_exr_passes(r._h, None, None, 0) == -1
    occ = upload(rec["occlusion"])
    assert call(None, 0, sources={"occlusion": occ.data_ptr() + 8})[0] == -1 and b"aligned" in L.rene_last_error()
    held = rec["direct"].copy()
    assert call(None, 0, sources={"direct": held.ctypes.data})[0] == -1 and b"rene_direct" in L.rene_last_error()  # host memory never reaches the kernel
    with api.Renderer(lights_scenes.cornell(W, H)) as fresh:
        assert code(lambda: fresh.exr_passes(layers="ao"), "rene_occlusion") == -1  # no library-owned result of that pass
        assert code(lambda: fresh.exr_passes_buffer()) == -1
        fresh.occlusion(0, 2)
        assert len(fresh.exr_passes(layers=("ao", "bent"))) > 0
        assert code(lambda: fresh.exr_passes(layers=("ao", "length")), "rene_bounces") == -1
        fresh.reset()
        assert code(lambda: fresh.exr_passes_buffer(), "reset") == -1  # the body is invalidated, the records are not
        assert len(fresh.exr_passes(layers="ao")) > 0
    with api.Renderer(lights_scenes.cornell(W, H), shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as part:
        part.render(0, 8)
        part.direct(0, 4)
        assert code(lambda: part.exr_passes_into(t, layers="indirect"), "frame shard") == -4
    assert (t == 0xAB).all().item()


def test_compressed_and_written_files(tmp_path):
    r, rec = job(0)
    mask, groups = abi.EXRP_ALL, 0
    attr_bytes, body_bytes, bpp = api.exr_passes_layout(W, H, mask, groups, NAMES)
    body = api.exr_passes_body_host(W, H, mask, groups, **rec)
    zips = r.exr_passes(path=str(tmp_path / "z.exr"), group_names=NAMES, compression="zips")
    assert (tmp_path / "z.exr").read_bytes() == zips and not (tmp_path / "z.exr.tmp").exists()
    same(zips, api.exr_passes_attributes(W, H, mask, groups, NAMES, "zips") + api.exr_compress_rows_host(W * bpp, H, attr_bytes, body, "zips"),
         "attributes + the host's chunks")
    plain = r.exr_passes(group_names=NAMES)
    assert len(zips) < len(plain)
    p, keep = api._exr_passes_params(mask, groups, NAMES)
    for compression, want in ((2, zips), (0, plain)):  # the library's own writer: the same files, through path + ".tmp"
        api._check(api.lib().rene_write_exr_passes(r._h, C.byref(p), compression, str(tmp_path / "w.exr").encode()))
        assert (tmp_path / "w.exr").read_bytes() == want and not (tmp_path / "w.exr.tmp").exists()
    assert api.lib().rene_write_exr_passes(r._h, C.byref(p), 2, str(tmp_path / "no" / "such" / "w.exr").encode()) == -6
    assert api.lib().rene_write_exr_passes(r._h, C.byref(p), 1, str(tmp_path / "w.exr").encode()) == -1

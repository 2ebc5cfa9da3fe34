"""GPU: the Cryptomatte output on the device (rene_output_cryptomatte, rene_exr_compress_rows, include/rene_hip.h).  The device's body is compared
BYTE FOR BYTE with the host's rene_cryptomatte_body_host on the records the device itself produced (tests/test_cryptomatte_host.py holds the host
form to an independent restatement), on a 70 x 45 film (partial tiles on both edges), a 64 x 32 film (whole tiles) and the crafted records; then what
the file MEANS is read back by an independent decoder: every name's matte is exactly its instances' share of the samples."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cryptomatte_reference as cr
from conftest import ROOT
from rene_amd import abi, api, loader

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
W, H, FRAMES = cr.FILM_W, cr.FILM_H, cr.FRAMES
DTYPE = np.dtype(abi.GBUFFER_DTYPE)


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


def records_into_tensor(r, ids, first=0, frames=FRAMES):
    """gbuffer_into a fresh tensor: (the tensor, its records on the host)."""
    import torch
    t = torch.empty(api.gbuffer_bytes(r.xres, r.yres), dtype=torch.uint8, device="cuda:0")
    r.gbuffer_into(t, first, frames, ids)
    return t, t.cpu().numpy().view(DTYPE).reshape(r.yres, r.xres)


def asset_names(scene):
    """A caller's own grouping over the instances: the wall, everything else that has a name, the strips."""
    return ["set" if n == "wall" else "strips" if n.startswith("object_") and i >= 6 else "props" for i, n in enumerate(scene.instance_names())]


class Job:
    def __init__(self, w, h):
        self.scene = cr.matte_scene(w, h)
        self.r = api.Renderer(self.scene)
        self.instance_tensor, self.instance_records = records_into_tensor(self.r, "instance")
        self.material_tensor, self.material_records = records_into_tensor(self.r, "material")
        own = self.r.gbuffer(0, FRAMES, "instance")  # the library-owned records: instance ids
        assert own.tobytes() == self.instance_records.tobytes()
        self.object = ("CryptoObject", "instance", self.scene.instance_names())
        self.material = ("CryptoMaterial", "material", self.scene.material_names())
        self.asset = ("CryptoAsset", "instance", asset_names(self.scene))

    def cases(self):
        """(described layers, the layers with their records for the device, the records on the host) for 1, 2 and 3 layers."""
        o, m, a = self.object, self.material, self.asset
        return {1: ([o], [o + (None,)], [self.instance_records]),
                2: ([o, m], [o + (None,), m + (self.material_tensor,)], [self.instance_records, self.material_records]),
                3: ([m, o, a], [m + (self.material_tensor,), o + (None,), a + (self.instance_tensor,)],
                    [self.material_records, self.instance_records, self.instance_records])}


@pytest.fixture(scope="module")
def job():
    j = Job(W, H)
    yield j
    j.r.close()


def test_the_scene_has_what_the_cases_need(job):
    rec = job.instance_records
    assert (rec["n"] == FRAMES).all() and (rec["hits"] == 0).any() and (rec["other"] > 0).any()  # the background; more ids than slots in a pixel
    pair = ((rec["id"] == 1) & (rec["count"] > 0)).any(-1) & ((rec["id"] == 2) & (rec["count"] > 0)).any(-1)
    assert pair.any(), "no pixel holds both instances of the shared name"
    assert ((rec["count"] > 0).sum(-1) == 4).any()


@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_device_body_equals_the_host_form(job, n_layers):
    import torch
    described, full, records = job.cases()[n_layers]
    want = api.cryptomatte_body_host(W, H, described, records)
    assert len(want) == api.cryptomatte_layout(W, H, described)[1]
    got = job.r.output_cryptomatte(full)
    same(got, want, f"{n_layers} layers, the library's buffer")
    assert job.r.cryptomatte_buffer()[1] == len(want)
    t = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert job.r.output_cryptomatte(full, t) is t
    host = t.cpu().numpy()
    same(host[:len(want)].tobytes(), want, f"{n_layers} layers, a caller's tensor")
    assert (host[len(want):] == 0xA5).all(), "bytes behind the body were written"
    assert job.instance_tensor.cpu().numpy().tobytes() == job.instance_records.tobytes()  # the records are read, not written
    assert job.r.gbuffer_buffer()[1] == W * H * 64 and api._download_result(job.r, api.lib().rene_download_gbuffer, (H, W), DTYPE).tobytes() == job.instance_records.tobytes()


def test_whole_tiles():
    """64 x 32: two whole tiles, every row a multiple of 64 lanes."""
    j = Job(64, 32)
    try:
        for n_layers, (described, full, records) in j.cases().items():
            same(j.r.output_cryptomatte(full), api.cryptomatte_body_host(64, 32, described, records), f"64 x 32, {n_layers} layers")
    finally:
        j.r.close()


def test_crafted_records():
    import torch
    rec = cr.crafted_records()
    flipped = rec[::-1, ::-1].copy()
    w, h = cr.CRAFTED_W, cr.CRAFTED_H
    o, m = ("CryptoObject", "instance", cr.CRAFTED_NAMES), ("CryptoMaterial", "material", cr.CRAFTED_MATERIAL_NAMES)
    with api.Renderer(cr.crafted_scene()) as r:
        t0 = torch.frombuffer(bytearray(rec.tobytes()), dtype=torch.uint8).to("cuda:0")
        t1 = torch.frombuffer(bytearray(flipped.tobytes()), dtype=torch.uint8).to("cuda:0")
        got = r.output_cryptomatte([o + (t0,), m + (t1,)])
        same(got, api.cryptomatte_body_host(w, h, [o, m], [rec, flipped]), "crafted records against the host form")
        same(got, cr.body(w, h, [o, m], [rec, flipped]), "crafted records against the restatement")
        same(r.output_cryptomatte([o + (t1,)]), cr.body(w, h, [o], [flipped]), "one layer")


def test_what_the_file_means(job):
    data = job.r.cryptomatte(compression="none")
    w, h, chans, attrs, compression, _ = cr.decode(data)
    assert (w, h, compression) == (W, H, 0)
    for (layer, ids, names), rec in ((job.object, job.instance_records), (job.material, job.material_records)):
        n = rec["n"].astype(np.float32)
        total = np.zeros((H, W), np.float32)
        for name in sorted(set(names)):
            mine = np.array([i for i, x in enumerate(names) if x == name], np.uint32)
            count = np.where(np.isin(rec["id"], mine), rec["count"], 0).sum(-1).astype(np.uint32)
            want = count.astype(np.float32) / n
            got = cr.matte(chans, layer, cr.name_hash(name))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (layer, name)
            total += got
        cov = np.stack([chans[f"{layer}{lv}.{c}"].view(np.float32) for lv, c in (("00", "G"), ("00", "A"), ("01", "G"), ("01", "A"))], -1)
        idb = np.stack([chans[f"{layer}{lv}.{c}"] for lv, c in (("00", "R"), ("00", "B"), ("01", "R"), ("01", "B"))], -1)
        assert (cov[..., :-1] >= cov[..., 1:]).all(), "coverages descend"
        assert (cov.astype(np.float64).sum(-1) <= rec["hits"] / rec["n"]).all() and np.array_equal(total, cov.sum(-1))  # (sixteenths: exact)
        assert ((cov == 0) == (idb == 0)).all(), "an unused rank is 0, 0"
        tie = (cov[..., :-1] == cov[..., 1:]) & (cov[..., 1:] > 0)
        assert (idb[..., :-1][tie] < idb[..., 1:][tie]).all(), "ties by key ascending"
    # the shared-name pair is ONE id: where both instances were hit, one rank holds their samples together
    rec = job.instance_records
    pair = ((rec["id"] == 1) & (rec["count"] > 0)).any(-1) & ((rec["id"] == 2) & (rec["count"] > 0)).any(-1)
    key = cr.name_hash("pair")
    ranks_with_key = sum((chans[f"CryptoObject{lv}.{c}"] == key).astype(int) for lv in ("00", "01") for c in "RB")
    assert (ranks_with_key[pair] == 1).all() and ranks_with_key.max() == 1
    both = np.where(np.isin(rec["id"], [1, 2]), rec["count"], 0).sum(-1)
    assert np.array_equal(cr.matte(chans, "CryptoObject", key)[pair], (both[pair] / np.float32(FRAMES)).astype(np.float32))
    # the manifest names the pair once, and every id in the file is in its layer's manifest
    by_name = {n: v for n, _, v in attrs}
    manifest = json.loads(by_name["cryptomatte/3ae39a5/manifest"].decode())
    assert list(manifest).count("pair") == 1 and manifest == cr.manifest_of(job.scene.instance_names())
    assert set(np.unique(idb)) - {0} <= {int(v, 16) for v in json.loads(by_name["cryptomatte/be359d6/manifest"].decode()).values()}


def test_compressed_and_written_files(job, tmp_path):
    r = job.r
    plain = r.cryptomatte(compression="none")
    described = [job.object, job.material]
    attr_bytes, body_bytes, bpp = api.cryptomatte_layout(W, H, described)
    body = api.cryptomatte_body_host(W, H, described, [job.instance_records, job.material_records])
    table = b"".join((attr_bytes + 8 * H + y * (8 + W * bpp)).to_bytes(8, "little") for y in range(H))
    same(plain, api.cryptomatte_attributes(W, H, described, "none") + table + body, "the uncompressed file is attributes + table + body")
    zips = r.cryptomatte(path=str(tmp_path / "z.exr"))
    assert (tmp_path / "z.exr").read_bytes() == zips and not (tmp_path / "z.exr.tmp").exists() and len(zips) < len(plain)
    cr.check_header(zips, W, H, described, 2)
    same(zips, api.cryptomatte_attributes(W, H, described, "zips") + api.exr_compress_rows_host(W * bpp, H, attr_bytes, body, "zips"), "the device's chunks are the host's")
    zw, zh, zchans, _, compression, _ = cr.decode(zips)  # (follows the table to every chunk and inflates it)
    pchans = cr.decode(plain)[2]
    assert (zw, zh, compression) == (W, H, 2) and all(np.array_equal(zchans[n], pchans[n]) for n in pchans)
    # the library's own writer: the same files, through path + ".tmp"
    arr, keep = api._cryptomatte_layers([job.object + (None,), job.material + (job.material_tensor.data_ptr(),)])
    p = abi.CryptomatteParams()
    api.lib().rene_cryptomatte_params_default(C.byref(p))
    p.n_layers, p.layers = 2, arr
    for compression, want in ((2, zips), (0, plain)):
        api._check(api.lib().rene_write_cryptomatte(r._h, C.byref(p), compression, str(tmp_path / "w.exr").encode()))
        assert (tmp_path / "w.exr").read_bytes() == want and not (tmp_path / "w.exr.tmp").exists()
    assert api.lib().rene_write_cryptomatte(r._h, C.byref(p), 2, str(tmp_path / "no" / "such" / "w.exr").encode()) == -6
    assert api.lib().rene_write_cryptomatte(r._h, C.byref(p), 1, str(tmp_path / "w.exr").encode()) == -1
    # names of the caller's own
    mine = r.cryptomatte(layers=("object",), names={"object": asset_names(job.scene)}, compression="none")
    manifest = json.loads({n: v for n, _, v in cr.decode(mine)[3]}["cryptomatte/3ae39a5/manifest"].decode())
    assert sorted(manifest) == ["props", "set", "strips"]


def test_two_tile_shards_fill_one_body(job):
    import torch
    described = [job.object, job.material]
    want = api.cryptomatte_body_host(W, H, described, [job.instance_records, job.material_records])
    attrs = api.cryptomatte_attributes(W, H, described, "zips")
    rs = [api.Renderer(job.scene, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=2) for k in range(2)]
    try:
        t = torch.full((len(want),), 0xAB, dtype=torch.uint8, device="cuda:0")
        for r in rs:
            assert r.cryptomatte_into(t) is t
            assert code(lambda: r.cryptomatte(), "shards") == -4
        same(t.cpu().numpy().tobytes(), want, "two shards' body")
        tail = rs[0].exr_compress_rows(W * 64, H, len(attrs), t)
        same(attrs + tail, job.r.cryptomatte(), "two shards' body, compressed by one")
        # a shard's own buffer holds its tiles' bytes and zeros elsewhere
        part = np.frombuffer(rs[1].output_cryptomatte([job.object + (None,)]), np.uint8)
        whole = np.frombuffer(api.cryptomatte_body_host(W, H, [job.object], [job.instance_records]), np.uint8)
        assert ((part == whole) | (part == 0)).all() and (part != whole).any() and part.any()
    finally:
        for r in rs:
            r.close()


def test_command_line(hip_lib, tmp_path):
    from test_cryptomatte_host import PBRT
    p = tmp_path / "scene.pbrt"
    p.write_text(PBRT)
    run = subprocess.run([CLI, str(p), "--spp", "8", "--cryptomatte", "crypto.exr", "--exr-compression", "zips"], capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 0, run.stderr
    info = [l for l in run.stderr.splitlines() if l.startswith("INFO cryptomatte")]
    assert len(info) == 1 and "CryptoObject 2 distinct names over 5 instances" in info[0] and "CryptoMaterial 3 distinct names over 3 materials" in info[0]
    got = (tmp_path / "crypto.exr").read_bytes()
    w, h, chans, attrs, compression, _ = cr.decode(got)
    assert (w, h, compression) == (24, 16, 2) and not (tmp_path / "crypto.exr.tmp").exists()
    manifest = {n: v for n, _, v in attrs}["cryptomatte/3ae39a5/manifest"].decode()
    assert manifest.count('"chair"') == 1 and json.loads(manifest) == cr.manifest_of(["chair", "object_4"])
    assert (chans["CryptoObject00.R"] == cr.name_hash("chair")).any()
    with api.Renderer(loader.load_pbrt(str(p))) as r:
        assert r.cryptomatte(n_frames=8) == got  # the Python route writes the same file
    run = subprocess.run([CLI, str(p), "--spp", "8", "--cryptomatte", "one.exr", "--cryptomatte-layers", "material", "--cryptomatte-frames", "4"],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 0, run.stderr
    w, h, chans, attrs, compression, _ = cr.decode((tmp_path / "one.exr").read_bytes())
    assert compression == 0 and list(chans) == cr.expected_channels(["CryptoMaterial"])
    for bad in (["--cryptomatte-layers", "primitive"], ["--cryptomatte-layers", "object,object"], ["--gpus", "2"]):
        assert subprocess.run([CLI, str(p), "--spp", "8", "--cryptomatte", "bad.exr"] + bad, capture_output=True, cwd=tmp_path).returncode == 2


def test_refusals_carry_messages(job):
    import torch
    o, m = job.object, job.material
    need = api.cryptomatte_layout(W, H, [o])[1]
    with api.Renderer(job.scene) as r:
        assert code(lambda: r.output_cryptomatte([o + (None,)]), "rene_gbuffer") == -1  # no geometry result yet
        assert code(lambda: r.cryptomatte_buffer()) == -1
        r.gbuffer(0, 4, "material")
        assert code(lambda: r.output_cryptomatte([o + (None,)]), "id_source") == -1  # the library-owned records hold material ids
        r.output_cryptomatte([m + (None,)], download=False)
        r.gbuffer(0, 4, "instance")
        assert code(lambda: r.output_cryptomatte([("CryptoObject", "instance", o[2][:-1], None)]), "n_names") == -1
        assert code(lambda: r.output_cryptomatte([("CryptoObject", "material", o[2], None)])) == -1
        t = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert code(lambda: r.output_cryptomatte([o + (None,)], t[:need - 1]), "dst_bytes") == -1
        assert code(lambda: r.output_cryptomatte([o + (None,)], t[2:]), "aligned") == -1
        assert (t == 0xA5).all().item(), "a refused call wrote"
        with pytest.raises((TypeError, ValueError)):
            r.output_cryptomatte([o + (None,)], t.cpu())
        L = api.lib()
        arr, keep = api._cryptomatte_layers([o + (None,)])
        p = abi.CryptomatteParams()
        L.rene_cryptomatte_params_default(C.byref(p))
        p.n_layers, p.layers = 1, arr
        host = np.full(need, 0xA5, np.uint8)
        assert L.rene_output_cryptomatte(r._h, C.byref(p), host.ctypes.data_as(C.c_void_p), need) == -1 and L.rene_last_error() and (host == 0xA5).all()
        host_records = job.instance_records.copy()
        arr[0].records = host_records.ctypes.data  # host memory as a layer's records never reaches the kernel
        assert L.rene_output_cryptomatte(r._h, C.byref(p), None, 0) == -1 and b"records" in L.rene_last_error()
        arr[0].records = job.instance_tensor.data_ptr() + 8
        assert L.rene_output_cryptomatte(r._h, C.byref(p), None, 0) == -1 and b"aligned" in L.rene_last_error()
        arr[0].records = None
        for field, bad in (("struct_size", 8), ("n_layers", 0), ("n_layers", 4), ("reserved", 1)):
            q = abi.CryptomatteParams()
            L.rene_cryptomatte_params_default(C.byref(q))
            q.n_layers, q.layers = 1, arr
            setattr(q, field, bad)
            assert L.rene_output_cryptomatte(r._h, C.byref(q), None, 0) == -1, field
        assert L.rene_output_cryptomatte(r._h, None, None, 0) == -1
        # use after rene_reset: the body is invalidated, the geometry records are not
        assert len(r.output_cryptomatte([o + (None,)])) == need
        r.reset()
        assert code(lambda: r.cryptomatte_buffer(), "reset") == -1
        assert code(lambda: api._download_result(r, L.rene_download_cryptomatte, (need,), np.uint8), "reset") == -1
        assert len(r.output_cryptomatte([o + (None,)])) == need

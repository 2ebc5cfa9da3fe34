"""CPU: the host side of the Cryptomatte output (include/rene_hip.h) against tests/cryptomatte_reference.py, which restates it independently -- the
hash and its known answers, the manifest, the file's layout and attributes walked by a parser of its own, rene_cryptomatte_body_host bit for bit on
crafted records, rene_exr_compress_rows_host against the mask-driven call and against zlib, the names the pbrt loader and the Python Scene keep, and
what must not have changed.  No GPU."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import cryptomatte_reference as cr
import exr_zips_reference as zr
from conftest import ROOT
from rene_amd import abi, api, loader

HEADER = os.path.join(ROOT, "include", "rene_hip.h")
OBJECT = ("CryptoObject", "instance", cr.CRAFTED_NAMES)
MATERIAL = ("CryptoMaterial", "material", cr.CRAFTED_MATERIAL_NAMES)
ASSET = ("CryptoAsset", "instance", ["a", "a", "b", "b", "c", "c", "d", "d"])  # a caller's own grouping over the instances

KNOWN = [("", 0x00800000), ("hello", 0x248BFA47), ("The quick brown fox jumps over the lazy dog", 0x2E4FF723), ("a", 0x3C2569B2), ("ab", 0x9BBFD75F),
         ("abc", 0xB3DD93FA), ("CryptoObject", 0x3AE39A58), ("CryptoMaterial", 0xBE359D67)]

PBRT = """Film "image" "integer xresolution" [ 24 ] "integer yresolution" [ 16 ] "string filename" [ "names.png" ]
LookAt 0 1 6.8  0 1 0  0 1 0
Camera "perspective" "float fov" [ 19.5 ]
WorldBegin
  MakeNamedMaterial "red paint" "string type" [ "matte" ] "rgb Kd" [ 0.6 0.1 0.1 ]
  ObjectBegin "chair"
    Shape "sphere" "float radius" [ 0.2 ]
    Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point P" [ -0.3 -0.3 0  0.3 -0.3 0  0 0.3 0 ]
  ObjectEnd
  AttributeBegin
    Translate -0.5 1 0
    ObjectInstance "chair"
  AttributeEnd
  AttributeBegin
    Translate 0.5 1 0
    ObjectInstance "chair"
  AttributeEnd
  Material "matte" "rgb Kd" [ 0.5 0.5 0.5 ]
  AttributeBegin
    AreaLightSource "diffuse" "rgb L" [ 5 5 5 ]
    Translate 0 1.8 0
    Shape "sphere" "float radius" [ 0.1 ]
  AttributeEnd
WorldEnd
"""


def code(fn):
    with pytest.raises(api.ReneError) as e:
        fn()
    assert str(e.value).split(": ", 1)[1].strip()  # a message
    return e.value.code


def test_hash_known_answers_and_the_float_fix(hip_lib):
    for name, want in KNOWN:
        assert api.cryptomatte_hash(name) == want == cr.name_hash(name), name
    assert cr.murmur3_32(b"") == 0 and cr.murmur3_32(b"hello") == 0x248BFA47  # the reference itself: the published vectors, unfixed
    rng = np.random.default_rng(11)
    for n in list(range(0, 14)) + [31, 64, 257]:  # every tail length, several blocks
        data = rng.integers(1, 256, n, dtype=np.uint8).tobytes()
        assert api.cryptomatte_hash(data) == cr.name_hash(data), n
    assert api.cryptomatte_hash("Bäume/木") == cr.name_hash("Bäume/木")  # UTF-8 bytes
    # a name whose raw hash has the exponent of an infinity or a NaN, found by search, is moved off it; so is one with a denormal's
    found = {}
    for i in range(4000):
        raw = cr.murmur3_32(b"object_%d" % i)
        e = (raw >> 23) & 255
        if e in (0, 255) and e not in found:
            found[e] = (b"object_%d" % i, raw)
    assert 255 in found, "no name of the search hashes to exponent 255"
    for e, (name, raw) in found.items():
        got = api.cryptomatte_hash(name)
        assert got == raw ^ (1 << 23) and (got >> 23) & 255 in (1, 254)
        assert np.isfinite(np.uint32(got).view(np.float32)) and abs(np.uint32(got).view(np.float32)) >= np.finfo(np.float32).tiny
    assert cr.layer_key("CryptoObject") == "3ae39a5" and cr.layer_key("CryptoMaterial") == "be359d6"


def test_manifest(hip_lib):
    names = cr.CRAFTED_MATERIAL_NAMES + ["\x01\x1f", "z z", "Bäume"]
    text = api.cryptomatte_manifest(names)
    assert text.encode(errors="surrogateescape") == cr.manifest_text(names)
    import json
    assert json.loads(text) == cr.manifest_of(names)
    assert '\\"hi\\"' in text and "back\\\\slash" in text and "\\u0009" in text and "\\u0001\\u001f" in text
    assert api.cryptomatte_manifest([]) == "{}" and api.cryptomatte_manifest(["a", "a"]) == '{"a":"3c2569b2"}'
    n = C.c_size_t()
    buf = C.create_string_buffer(4)
    assert api.lib().rene_cryptomatte_manifest((C.c_char_p * 1)(b"abc"), 1, buf, 4, C.byref(n)) == -1 and n.value == len('{"abc":"b3dd93fa"}')
    assert api.lib().rene_cryptomatte_manifest((C.c_char_p * 1)(None), 1, None, 0, C.byref(n)) == -1


@pytest.mark.parametrize("layers", [[OBJECT], [OBJECT, MATERIAL], [MATERIAL, OBJECT, ASSET]], ids=["1", "2", "3"])
def test_layout_and_attributes(hip_lib, layers):
    w, h = 5, 3
    attr_bytes, body_bytes, bpp = api.cryptomatte_layout(w, h, layers)
    assert bpp == 32 * len(layers) and body_bytes == h * (8 + w * bpp)
    for compression, byte in (("none", 0), ("zips", 2)):
        a = api.cryptomatte_attributes(w, h, layers, compression)
        assert len(a) == attr_bytes and cr.check_header(a, w, h, layers, byte) == attr_bytes
    # the whole uncompressed file: attributes + 8 H of table + body, and an independent reader decodes it
    recs = [cr.crafted_records()] * len(layers)
    body = api.cryptomatte_body_host(w, h, layers, recs)
    tail = api.exr_compress_rows_host(w * bpp, h, attr_bytes, body, "none")
    data = api.cryptomatte_attributes(w, h, layers, "none") + tail
    assert len(data) == attr_bytes + 8 * h + body_bytes
    dw, dh, chans, _, compression, table = cr.decode(data)
    assert (dw, dh, compression) == (w, h, 0) and table == [attr_bytes + 8 * h + y * (8 + w * bpp) for y in range(h)]
    assert list(chans) == cr.expected_channels([L[0] for L in layers])


def test_channel_rows_follow_the_bytes_of_interleaving_names(hip_lib):
    """"A" and "A00B" are both legal names, and "A00B00.x" lies between "A00.x" and "A01.x": the chunk's rows are in the channel list's order."""
    layers = [("A00B", "instance", cr.CRAFTED_NAMES), ("A", "material", cr.CRAFTED_MATERIAL_NAMES)]
    order = cr.expected_channels(["A00B", "A"])
    assert order[:4] == ["A00.A", "A00.B", "A00.G", "A00.R"] and order[4].startswith("A00B00") and order[-1] == "A01.R"
    a = api.cryptomatte_attributes(5, 3, layers, "none")
    cr.check_header(a, 5, 3, layers, 0)
    rec = cr.crafted_records()
    assert api.cryptomatte_body_host(5, 3, layers, [rec, rec]) == cr.body(5, 3, layers, [rec, rec])


def test_refusals(hip_lib):
    ok = cr.CRAFTED_NAMES
    for name in ("", "Crypto1", "Crypto Object", "Crypto.Object", "x" * 25, "Cryptö"):
        assert code(lambda: api.cryptomatte_layout(4, 4, [(name, "instance", ok)])) == -1, name
    assert api.cryptomatte_layout(4, 4, [("x" * 24, "instance", ok)])[2] == 32 and api.cryptomatte_layout(4, 4, [("a1_b", "instance", ok)])[2] == 32
    assert code(lambda: api.cryptomatte_layout(4, 4, [OBJECT, OBJECT])) == -1  # one name twice (and so one key)
    assert code(lambda: api.cryptomatte_layout(4, 4, [OBJECT, MATERIAL, ASSET, ("More", "instance", ok)])) == -1
    assert code(lambda: api.cryptomatte_layout(4, 4, [])) == -1
    for w, h in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        assert code(lambda: api.cryptomatte_layout(w, h, [OBJECT])) == -1
    assert api.cryptomatte_layout(16384, 16384, [OBJECT])[1] == 16384 * (8 + 16384 * 32)
    # _PRIMITIVE has no names; an unknown source; a NULL name; the host body without records, or a short destination
    L = api.lib()
    arr, keep = api._cryptomatte_host_layers([OBJECT])
    n = C.c_size_t()
    for source in (abi.GBUFFER_ID_PRIMITIVE, 3):
        arr[0].id_source = source
        assert L.rene_cryptomatte_layout(4, 4, arr, 1, C.byref(n), None, None) == -1 and b"id_source" in L.rene_last_error()
    arr[0].id_source = abi.GBUFFER_ID_INSTANCE
    assert L.rene_cryptomatte_layout(4, 4, arr, 1, C.byref(n), None, None) == 0
    arr[0].names[2] = None
    assert L.rene_cryptomatte_layout(4, 4, arr, 1, C.byref(n), None, None) == -1
    assert L.rene_cryptomatte_layout(4, 4, None, 1, C.byref(n), None, None) == -1
    assert code(lambda: api.cryptomatte_attributes(4, 4, [OBJECT], 3)) == -1
    arr, keep = api._cryptomatte_host_layers([OBJECT])
    rec = cr.crafted_records()
    ptrs = (C.c_void_p * 1)(rec.ctypes.data)
    out = np.zeros(3 * (8 + 5 * 32), np.uint8)
    assert L.rene_cryptomatte_body_host(5, 3, arr, 1, ptrs, out.ctypes.data_as(C.c_void_p), out.size - 1) == -1 and not out.any()
    assert L.rene_cryptomatte_body_host(5, 3, arr, 1, (C.c_void_p * 1)(None), out.ctypes.data_as(C.c_void_p), out.size) == -1
    assert L.rene_cryptomatte_body_host(5, 3, arr, 1, ptrs, out.ctypes.data_as(C.c_void_p), out.size) == 0 and out.any()


@pytest.mark.parametrize("layers", [[OBJECT], [OBJECT, MATERIAL], [MATERIAL, OBJECT, ASSET]], ids=["1", "2", "3"])
def test_body_host_equals_the_numpy_restatement(hip_lib, layers):
    rec = cr.crafted_records()
    recs = [rec, rec[::-1, ::-1].copy(), rec][:len(layers)]
    got, want = api.cryptomatte_body_host(cr.CRAFTED_W, cr.CRAFTED_H, layers, recs), cr.body(cr.CRAFTED_W, cr.CRAFTED_H, layers, recs)
    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert len(got) == len(want) and bad.size == 0, bad[:8].tolist()


def test_the_crafted_cases_mean_what_their_comments_say():
    """The restatement itself, on the cases by hand."""
    flat = cr.crafted_records().reshape(-1)
    ball, wall, lamp, floor = (cr.name_hash(n) for n in ("ball", "wall", "lamp", "floor"))
    f = np.float32
    assert cr.ranks(flat[0], cr.CRAFTED_NAMES) == [(0, f(0))] * 4
    assert cr.ranks(flat[1], cr.CRAFTED_NAMES) == [(ball, f(14) / f(16))] + [(0, f(0))] * 3
    assert cr.ranks(flat[2], cr.CRAFTED_NAMES)[:2] == [(ball, f(6) / f(16)), (wall, f(5) / f(16))]
    assert [k for k, _ in cr.ranks(flat[3], cr.CRAFTED_NAMES)[:3]] == sorted([wall, lamp, floor])
    assert cr.ranks(flat[4], cr.CRAFTED_NAMES) == [(wall, f(5) / f(16)), (lamp, f(3) / f(16)), (0, f(0)), (0, f(0))]
    assert [k for k, _ in cr.ranks(flat[5], cr.CRAFTED_NAMES)] == [wall, floor, ball, 0]
    assert cr.ranks(flat[7], cr.CRAFTED_NAMES)[0] == (ball, f(6) / f(16))
    assert cr.ranks(flat[14], cr.CRAFTED_NAMES)[0] == (ball, f(1) / f(0xFFFFFFFF))  # (2^32 - 1) + 2 wraps to 1
    for p in range(flat.size):  # coverages descend, ids of used ranks are distinct
        rk = cr.ranks(flat[p], cr.CRAFTED_NAMES)
        cov = [c for _, c in rk]
        used = [k for k, c in rk if c > 0]
        assert cov == sorted(cov, reverse=True) and len(set(used)) == len(used)


def test_compress_rows_host(hip_lib):
    # with a mask's row bytes and attribute size: the bytes of rene_exr_compress_host
    for name, w, h, mask, body in zr.cpu_cases()[:9]:
        head = api.exr_layout(w, h, mask)[0] - 8 * h
        row = w * zr.bytes_per_pixel(mask)
        for compression in ("zips", "none"):
            assert api.exr_compress_rows_host(row, h, head, body, compression) == api.exr_compress_host(w, h, mask, body, compression), (name, compression)
    # a Cryptomatte body: every chunk inflates and un-preprocesses back to the body's row
    layers = [OBJECT, MATERIAL]
    w, h = cr.CRAFTED_W, cr.CRAFTED_H
    rec = cr.crafted_records()
    body = api.cryptomatte_body_host(w, h, layers, [rec, rec])
    attrs = api.cryptomatte_attributes(w, h, layers, "zips")
    tail = api.exr_compress_rows_host(w * 64, h, len(attrs), body, "zips")
    at = 8 * h
    for y in range(h):
        assert struct.unpack_from("<Q", tail, 8 * y)[0] == len(attrs) + at
        yy, size = struct.unpack_from("<ii", tail, at)
        raw = body[y * (8 + w * 64) + 8:(y + 1) * (8 + w * 64)]
        assert yy == y and 0 < size <= len(raw)
        chunk = tail[at + 8:at + 8 + size]
        assert (chunk == raw) if size == len(raw) else (zr.raw_from_d(np.frombuffer(zlib.decompress(chunk), np.uint8)) == raw)
        at += 8 + size
    assert at == len(tail)
    dw, dh, chans, _, compression, _ = cr.decode(attrs + tail)
    assert compression == 2 and chans["CryptoObject00.R"].tobytes() == cr.decode(api.cryptomatte_attributes(w, h, layers, "none") +
                                                                                api.exr_compress_rows_host(w * 64, h, len(attrs), body, "none"))[2]["CryptoObject00.R"].tobytes()
    # refusals
    for row, hh, nbytes in ((0, h, len(body)), (w * 64 + 1, h, len(body)), (16384 * 96 + 2, 1, 16384 * 96 + 10), (w * 64, 0, len(body)), (w * 64, 16385, len(body)),
                            (w * 64, h, len(body) - 1)):
        assert code(lambda: api.exr_compress_rows_host(row, hh, len(attrs), body[:nbytes] if nbytes <= len(body) else body + bytes(nbytes - len(body)), "zips")) == -1, (row, hh)
    assert code(lambda: api.exr_compress_rows_host(w * 64, h, len(attrs), body, 1)) == -1


def test_names_of_a_loaded_scene_and_of_a_python_scene(hip_lib):
    s = loader.parse_pbrt(PBRT)
    # two instancings of an object of two shapes, then a top-level shape; the index-0 material, a named one, an anonymous one
    assert s.instance_names() == ["chair", "chair", "chair", "chair", "object_4"]
    assert s.material_names() == ["material_0", "red paint", "material_2"]
    assert api.lib().rene_scene_instance_name(s._h, 5) is None and api.lib().rene_scene_material_name(s._h, 3) is None
    assert api.lib().rene_scene_instance_name(None, 0) is None
    py = cr.matte_scene()
    assert py.instance_names()[:6] == ["wall", "pair", "pair", "ball", "object_4", "lamp"] and py.instance_names()[6] == "object_6"
    assert py.material_names() == ["material_0", "plaster", "red paint", "material_3", "material_4", "material_5"]
    assert len(py.instance_names()) == len(py.instances) and len(py.material_names()) == len(py.materials)
    described = api.cryptomatte_scene_layers(("object", "material"), lambda layer: {"object": py.instance_names(), "material": py.material_names()}[layer])
    assert [d[:2] for d in described] == [("CryptoObject", "instance"), ("CryptoMaterial", "material")]
    with pytest.raises(ValueError):
        api.cryptomatte_scene_layers(("primitive",), lambda layer: [])


def test_what_has_not_changed(hip_lib, tmp_path):
    assert hip_lib.rene_abi_version() == abi.ABI_VERSION == 7
    names = ("rene_scene_desc", "rene_exr_params", "rene_gbuffer_params", "rene_gbuffer_pixel", "rene_cryptomatte_layer", "rene_cryptomatte_params")
    prog = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){\n' + "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in names) + "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])  # the header stays C99
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert sizes[:4] == [328, 16, 20, 64], "rene_scene_desc, rene_exr_params, rene_gbuffer_params and the record are what they were"
    assert sizes[:3] == [C.sizeof(abi.SceneDesc), C.sizeof(abi.ExrParams), C.sizeof(abi.GbufferParams)]
    assert sizes[4:] == [C.sizeof(abi.CryptomatteLayer), C.sizeof(abi.CryptomatteParams)]
    assert abi.EXR_ALL == 255 and code(lambda: api.exr_layout(4, 4, 256)) == -1 and code(lambda: api.exr_header(4, 4, 256)) == -1
    for sym in ("rene_cryptomatte_params_default", "rene_cryptomatte_hash", "rene_cryptomatte_manifest", "rene_cryptomatte_layout", "rene_cryptomatte_attributes",
                "rene_cryptomatte_body_host", "rene_output_cryptomatte", "rene_cryptomatte_buffer", "rene_download_cryptomatte", "rene_write_cryptomatte",
                "rene_exr_compress_rows", "rene_exr_compress_rows_host", "rene_scene_instance_name", "rene_scene_material_name"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, sym), sym
    p = abi.CryptomatteParams()
    hip_lib.rene_cryptomatte_params_default(C.byref(p))
    assert (p.struct_size, p.n_layers, p.reserved) == (C.sizeof(abi.CryptomatteParams), 0, 0) and not p.layers
    # the device calls refuse a NULL context before anything touches a device
    assert hip_lib.rene_output_cryptomatte(None, C.byref(p), None, 0) == -1 and hip_lib.rene_write_cryptomatte(None, C.byref(p), 2, b"x") == -1
    n = C.c_size_t()
    assert hip_lib.rene_exr_compress_rows(None, 64, 1, 300, 2, None, 72, None, 0, C.byref(n)) == -1
    assert hip_lib.rene_cryptomatte_buffer(None, None, None) == -1 and hip_lib.rene_download_cryptomatte(None, None, 0) == -1


def test_kernel_resources():
    """The pack keeps its four (count, key) pairs per layer in registers: no scratch, no LDS (tools/res_summary.py reads the same file)."""
    res = os.path.join(ROOT, "rene_amd", "csrc", "kernels_cryptomatte.res")
    if not os.path.exists(res):
        api.build()
    text = open(res).read()
    assert text.count("Function Name:") == 1 and "cryptomatte_kernel" in text
    assert "ScratchSize [bytes/lane]: 0 " in text and "LDS Size [bytes/block]: 0 " in text and "VGPRs Spill: 0 " in text

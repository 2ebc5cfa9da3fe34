"""CPU: the host side of the pass-layer OpenEXR file (rene_exr_passes_layout, rene_exr_passes_attributes, rene_exr_passes_body_host,
include/rene_hip.h) against tests/exr_passes_reference.py, an independent numpy writer: the header and the body byte for byte on crafted records
salted with the edges, the layout of all 127 layer masks, the rene/lightGroups attribute, every host-side refusal, the command line's options, the
file read back by the tests' own OpenEXR parser, and every ZIPS chunk inflated by zlib.  No GPU."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import cryptomatte_reference as cr
import exr_passes_reference as pr
import exr_reference
import exr_zips_reference as zr
from conftest import ROOT
from rene_amd import abi, api

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
CLI = os.path.join(CSRC, "rene-hip")
HEADER = os.path.join(ROOT, "include", "rene_hip.h")
ALL = abi.EXRP_ALL
NAMES = ["sky", None, "key light", "rim-2", None, None, None, "fill_7"]
FILMS = [(1, 1), (33, 2), (33, 3), (77, 45)]
_crafted = {}


def crafted(w, h):
    if (w, h) not in _crafted:
        _crafted[w, h] = pr.crafted(w, h)
    return _crafted[w, h]


def code(fn):
    with pytest.raises(api.ReneError) as e:
        fn()
    assert str(e.value).split(": ", 1)[1].strip()  # a message
    return e.value.code


def same(got, want, label):
    assert len(got) == len(want), (label, len(got), len(want))
    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert bad.size == 0, (label, len(bad), bad[:8].tolist())


def host_file(w, h, mask, groups, names, **sources):
    attrs = api.exr_passes_attributes(w, h, mask, groups, names)
    bpp = api.exr_passes_layout(w, h, mask, groups, names)[2]
    return attrs + api.exr_passes_table(w, h, len(attrs), bpp) + api.exr_passes_body_host(w, h, mask, groups, **sources)


@pytest.mark.parametrize("w,h", FILMS)
def test_header_and_body_are_the_reference_writers(hip_lib, w, h):
    c = crafted(w, h)
    cases = [(ALL, 0, NAMES), (abi.EXRP_AO, 0, None), (abi.EXRP_AO | abi.EXRP_BENT, 0, None), (abi.EXRP_LIGHTS, 0x0A, NAMES), (abi.EXRP_INDIRECT, 0, None),
             (abi.EXRP_BOUNCES | abi.EXRP_LENGTH, 0, None), (abi.EXRP_DIRECT | abi.EXRP_LIGHTS, 0x81, None)]
    for mask, groups, names in cases:
        same(host_file(w, h, mask, groups, names, **c), pr.file_bytes(w, h, mask, groups, names, **c), (w, h, mask, groups))
    if w == 33:  # `ao` alone: bpp 2, a chunk of 74 bytes -- every odd row starts at an address = 2 (mod 4); `ao + bent`: bpp 8, everything aligned
        assert api.exr_passes_layout(w, h, "ao")[1:] == (h * 74, 2) and (8 + w * 2) % 4 == 2
        assert api.exr_passes_layout(w, h, ("ao", "bent"))[1:] == (h * (8 + 33 * 8), 8)


def test_the_crafted_records_hold_the_edges():
    c = crafted(33, 2)
    p = pr.planes(ALL, 0, **c)
    bits = {k: pr.half_bits(v) for k, v in p.items()}
    every = np.concatenate([b.reshape(-1) for b in bits.values()])
    values = np.concatenate([v.reshape(-1) for v in p.values()])
    assert (c["direct"]["n"] == 0).any() and (c["occlusion"]["rays"] == 0).any() and (c["bounces"]["n"] == 0).any() and (c["lights"]["n"] == 0).any()
    assert (c["occlusion"]["bent_sum"] == 0).all(-1).any()
    assert np.isnan(values).any() and np.isposinf(values).any() and np.isneginf(values).any() and (every == 0x7E00).any()
    assert (values > 65504).any() and (every == 0x7BFF).any() and (every == 0xFBFF).any()  # clamped to the largest half
    assert ((every & 0x7FFF) > 0).any() and (((every & 0x7C00) == 0) & ((every & 0x3FF) != 0)).any()  # half subnormals
    assert ((values == np.float32(2.0 ** -25)) & True).any() and (every == 0x8000).any()  # the tie below the smallest subnormal; -0.0
    assert (p["indirect.R"] < 0).any() or (p["indirect.G"] < 0).any() or (p["indirect.B"] < 0).any()
    assert (p["ao"] == 1).any() and (p["ao"] == 0).any() and not np.isnan(p["bent.X"][0, 2])  # (a NaN length gives 0)
    assert bits["bent.X"].reshape(-1)[5] == 0x3C00  # 1e-20: its square is an fp32 denormal, kept


def test_layout_of_every_mask(hip_lib):
    w, h = 77, 45
    for mask in range(1, 128):
        for groups in (0, 1, 0x81, 0xFF):
            if groups and not mask & abi.EXRP_LIGHTS:
                assert code(lambda: api.exr_passes_layout(w, h, mask, groups)) == -1
                continue
            attr, body, bpp = api.exr_passes_layout(w, h, mask, groups)
            ref = pr.attributes(w, h, mask, groups)
            assert (attr, body, bpp) == (len(ref), h * (8 + w * pr.bytes_per_pixel(mask, groups)), pr.bytes_per_pixel(mask, groups)), (mask, groups)
            assert 2 <= bpp <= 130
            if mask in (1, 5, 32, 64, 127):
                assert api.exr_passes_attributes(w, h, mask, groups) == ref
                names = [n for n, _ in cr.channel_list({n: v for n, _, v in cr.walk_header(ref)[0]}["channels"])]
                assert names == pr.channel_names(mask, groups) == sorted(names, key=lambda s: s.encode())
    assert api.exr_passes_layout(1, 1, ALL)[2] == 130 and api.exr_passes_layout(16384, 16384, "ao")[1] == 16384 * (8 + 2 * 16384)
    p = abi.ExrPassesParams()
    hip_lib.rene_exr_passes_params_default(C.byref(p))
    assert (p.struct_size, p.layers, p.groups, p.reserved) == (C.sizeof(abi.ExrPassesParams), 127, 0, 0)
    assert not p.group_names and not p.occlusion and not p.direct and not p.bounces and not p.lights


def test_light_group_names(hip_lib):
    w, h = 8, 4
    plain = api.exr_passes_attributes(w, h, "lights")
    named = api.exr_passes_attributes(w, h, "lights", None, NAMES)
    attrs, end = cr.walk_header(named)
    assert end == len(named) and [n for n, _, _ in attrs][:8] == [n for n, _, _ in cr.walk_header(plain)[0]] and len(cr.walk_header(plain)[0]) == 8
    assert attrs[8] == ("rene/lightGroups", "string", b'{"light0":"sky","light2":"key light","light3":"rim-2","light7":"fill_7"}')
    assert named == pr.attributes(w, h, abi.EXRP_LIGHTS, 0, NAMES)
    assert api.exr_passes_layout(w, h, "lights", None, NAMES)[0] == len(named) == len(plain) + len(b"rene/lightGroups\0string\0") + 4 + len(attrs[8][2])
    # only the groups that are written, in group order; no written group with a name: no attribute
    assert cr.walk_header(api.exr_passes_attributes(w, h, "lights", 0x0C, NAMES))[0][8][2] == b'{"light2":"key light","light3":"rim-2"}'
    assert api.exr_passes_attributes(w, h, "lights", 0x12, NAMES) == api.exr_passes_attributes(w, h, "lights", 0x12)
    assert api.exr_passes_attributes(w, h, ("ao", "direct"), None, NAMES) == api.exr_passes_attributes(w, h, ("ao", "direct"))
    assert api.exr_passes_attributes(w, h, "lights", None, {3: "rim-2"}) == pr.attributes(w, h, abi.EXRP_LIGHTS, 0, [None, None, None, "rim-2"] + [None] * 4)
    # the escapes of the manifest have no case: the bytes that would need them are refused, a group's that is not written too
    for bad in ('a"b', "a\\b", "tab\t", "", "x" * 25, "café", "a,b", "a:b"):
        assert code(lambda: api.exr_passes_layout(w, h, "lights", 1, [None, bad] + [None] * 6)) == -1, bad
    assert api.exr_passes_layout(w, h, "lights", None, ["x" * 24] + [None] * 7)[0] == len(plain) + len(b"rene/lightGroups\0string\0") + 4 + len(b'{"light0":""}') + 24


def test_refusals(hip_lib):
    c = crafted(33, 2)
    w, h = 33, 2
    L = hip_lib
    for call in (lambda: api.exr_passes_layout(w, h, 0), lambda: api.exr_passes_layout(w, h, 128), lambda: api.exr_passes_layout(w, h, "ao", 1),
                 lambda: api.exr_passes_layout(w, h, "lights", 256), lambda: api.exr_passes_layout(0, h), lambda: api.exr_passes_layout(w, 16385),
                 lambda: api.exr_passes_layout(16385, 1), lambda: api.exr_passes_attributes(w, h, "ao", compression=1),
                 lambda: api.exr_passes_body_host(w, h, "ao"), lambda: api.exr_passes_body_host(w, h, "length", direct=c["direct"]),
                 lambda: api.exr_passes_body_host(w, h, "indirect", direct=c["direct"]), lambda: api.exr_passes_body_host(w, h, "lights", bounces=c["bounces"])):
        assert code(call) == -1
    with pytest.raises(ValueError):
        api.exr_passes_mask(("ao", "beauty"))
    with pytest.raises(ValueError):
        api.exr_passes_body_host(w, h, "ao", occlusion=c["occlusion"][:1])
    with pytest.raises(TypeError):
        api.exr_passes_body_host(w, h, "ao", occlusion=c["direct"])
    assert api.exr_passes_mask(("ao", "lights")) == abi.EXRP_AO | abi.EXRP_LIGHTS and api.exr_passes_mask("length") == abi.EXRP_LENGTH
    p, keep = api._exr_passes_params(ALL, None, None)
    n = C.c_size_t()
    for field, bad in (("struct_size", 8), ("reserved", 1)):
        q, _ = api._exr_passes_params(ALL, None, None)
        setattr(q, field, bad)
        assert L.rene_exr_passes_layout(w, h, C.byref(q), C.byref(n), None, None) == -1, field
    assert L.rene_exr_passes_layout(w, h, None, C.byref(n), None, None) == -1
    assert L.rene_exr_passes_layout(w, h, C.byref(p), None, None, None) == 0  # (every out-pointer is optional)
    buf = C.create_string_buffer(4096)
    assert L.rene_exr_passes_attributes(w, h, C.byref(p), 0, None, 4096) == -1 and L.rene_exr_passes_attributes(w, h, C.byref(p), 0, buf, 16) == -1
    q, keep = api._exr_passes_params("ao", None, None, {"occlusion": c["occlusion"].ctypes.data})
    need = api.exr_passes_layout(w, h, "ao")[1]
    out = np.full(need, 0xAB, np.uint8)
    assert L.rene_exr_passes_body_host(w, h, C.byref(q), None, out.ctypes.data_as(C.c_void_p), need - 1) == -1 and (out == 0xAB).all()
    assert L.rene_exr_passes_body_host(w, h, C.byref(q), None, None, need) == -1
    assert L.rene_exr_passes_body_host(w, h, C.byref(q), None, out.ctypes.data_as(C.c_void_p), need) == 0
    # the device calls refuse a NULL context or NULL params before anything touches a device
    assert L.rene_output_exr_passes(None, C.byref(p), None, 0) == -1 and L.rene_write_exr_passes(None, C.byref(p), 2, b"x") == -1
    assert L.rene_exr_passes_buffer(None, None, None) == -1 and L.rene_download_exr_passes(None, None, 0) == -1


def test_a_reader_gets_the_rounded_planes_back(hip_lib):
    w, h = 33, 3
    c = crafted(w, h)
    data = host_file(w, h, ALL, 0x2D, NAMES, **c)
    pw, ph, chans = exr_reference.parse(data)  # follows every offset of the table
    want = pr.planes(ALL, 0x2D, **c)
    assert (pw, ph) == (w, h) and list(chans) == pr.channel_names(ALL, 0x2D) and len(chans) == 1 + 3 + 30 + 3 + 3 + 12 + 1
    for name, plane in chans.items():
        assert plane.dtype == np.dtype("<f2") and plane.view(np.uint16).tobytes() == pr.half_bits(want[name]).tobytes(), name
    some = chans["depth3.G"].astype(np.float32)
    with np.errstate(all="ignore"):
        near = np.isfinite(want["depth3.G"]) & (np.abs(want["depth3.G"]) < 60000) & (np.abs(want["depth3.G"]) > 1e-3)
        assert near.any() and (np.abs(some[near] - want["depth3.G"][near]) <= np.abs(want["depth3.G"][near]) * 2.0 ** -11).all()


def test_every_zips_chunk_inflates(hip_lib):
    w, h = 77, 45
    c = crafted(w, h)
    mask, groups = ALL, 0
    attrs = api.exr_passes_attributes(w, h, mask, groups, NAMES, "zips")
    assert cr.walk_header(attrs)[0][1] == ("compression", "compression", b"\x02")
    body = api.exr_passes_body_host(w, h, mask, groups, **c)
    row = w * 130
    tail = api.exr_compress_rows_host(row, h, len(attrs), body, "zips")
    table = struct.unpack_from(f"<{h}Q", tail, 0)
    end = len(attrs) + 8 * h
    for y in range(h):
        assert table[y] == end
        at = end - len(attrs)
        yy, size = struct.unpack_from("<ii", tail, at)
        assert yy == y and 0 < size <= row
        raw = tail[at + 8:at + 8 + size]
        if size != row:
            raw = bytes(zr.raw_from_d(np.frombuffer(zlib.decompress(raw), np.uint8)))
        assert bytes(raw) == body[y * (8 + row) + 8:(y + 1) * (8 + row)], y
        end += 8 + size
    assert end == len(attrs) + len(tail)


def test_cli_options(hip_lib, tmp_path):
    if not os.path.exists(CLI):
        api.build()
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, cwd=tmp_path)
    missing = str(tmp_path / "missing.pbrt")
    r = run("--help")
    assert "--exr-passes PATH" in r.stderr and "--exr-pass-layers" in r.stderr and "--exr-light-names" in r.stderr
    # the options parse: the run gets as far as the scene file
    for extra in ([], ["--exr-pass-layers", "ao"], ["--exr-pass-layers", "ao,bent,direct,indirect,bounces,length,lights"], ["--exr-compression", "zips"],
                  ["--exr-light-names", "sky,,key light,rim-2"], ["--ao", "a", "--ao-rays", "4", "--ao-radius", "0.5"], ["--bounces-max-depth", "6"],
                  ["--exr-pass-layers", "direct,lights", "--adaptive", "--target-noise", "0.1"], ["--exr", "o.exr", "--exr-layers", "beauty"]):
        r = run(missing, "--exr-passes", "p.exr", *extra)
        assert r.returncode == 1 and "cannot open" in r.stdout and "unknown option" not in r.stderr, (extra, r.stderr)
    for extra, word in ((["--exr-pass-layers", "ao,colour"], "unknown layer 'colour'"), (["--exr-pass-layers", "ao,"], "unknown layer ''"), (["--gpus", "2"], "--gpus 2"),
                        (["--adaptive", "--target-noise", "0.1"], "indirect"), (["--exr-pass-layers", "indirect", "--adaptive", "--target-noise", "0.1"], "indirect"),
                        (["--exr-light-names", 'a"b'], "--exr-light-names"), (["--exr-light-names", "a,b,c,d,e,f,g,h,i"], "--exr-light-names"),
                        (["--exr-pass-layers", "ao", "--exr-light-names", "a"], "lights layer"), (["--ao-rays", "65"], "--ao-rays"),
                        (["--bounces-max-depth", "51"], "--bounces-max-depth"), (["--exr-compression", "piz"], "unknown compression")):
        r = run(missing, "--exr-passes", "p.exr", *extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
    for lone in (["--exr-pass-layers", "ao"], ["--exr-light-names", "a"]):
        r = run(missing, *lone)
        assert r.returncode == 2 and "need --exr-passes" in r.stderr
    assert run(missing, "--exr-compression", "zips").returncode == 2


def test_the_unit_its_flags_and_its_shared_store():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_exr_passes.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    rule = re.search(r"^kernels_exr_passes\.o: kernels_exr_passes\.hip \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(ROBUSTFLAGS)" in rule and "$(HIPFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_exr_passes.res" in rule
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert "$(ROBUSTFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_exr_passes.o kernels_exr_passes.hip" in variant
    assert "exr_store.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    for unit in ("kernels_exr.hip", "kernels_exr_passes.hip"):  # one two-halves store, in one header
        src = open(os.path.join(CSRC, unit)).read()
        assert '#include "exr_store.h"' in src and "void store_word(" not in src and '#include "half_element.h"' in src, unit
    src = open(os.path.join(CSRC, "kernels_exr_passes.hip")).read()
    code_lines = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "atomic" not in code_lines and "__shared__" not in code_lines and code_lines.count("__global__") == 1 and "template" not in code_lines  # one kernel, no instantiation per mask


def test_what_has_not_changed(hip_lib, tmp_path):
    assert hip_lib.rene_abi_version() == abi.ABI_VERSION == 7
    names = ("rene_exr_params", "rene_cryptomatte_params", "rene_occlusion_pixel", "rene_direct_pixel", "rene_bounces_pixel", "rene_lights_pixel", "rene_exr_passes_params")
    prog = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){\n' + "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in names) + "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])  # the header stays C99
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert sizes == [C.sizeof(abi.ExrParams), C.sizeof(abi.CryptomatteParams), 32, 48, 176, 144, C.sizeof(abi.ExrPassesParams)]
    assert abi.EXR_ALL == 255 and code(lambda: api.exr_layout(4, 4, 256)) == -1 and abi.EXRP_ALL == 127
    for sym in ("rene_exr_passes_params_default", "rene_exr_passes_layout", "rene_exr_passes_attributes", "rene_exr_passes_body_host", "rene_output_exr_passes",
                "rene_exr_passes_buffer", "rene_download_exr_passes", "rene_write_exr_passes"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, sym), sym

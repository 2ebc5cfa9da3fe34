"""Test helper (not a conftest): the Cryptomatte output (rene_output_cryptomatte, include/rene_hip.h) restated independently of the library --
MurmurHash3_x86_32 and the float fix in pure Python, the manifest, a walker over an OpenEXR header, the body's values per pixel by the header's six
rules in numpy, a decoder of a whole file (uncompressed or ZIPS) -- and the inputs the CPU and the GPU tests share: the crafted records at 5 x 3
with a scene of that film and as many instances, and the 70 x 45 scene of quads and spheres."""
import json
import struct
import zlib

import numpy as np

import exr_zips_reference as zr
from rene_amd import abi, glam, scenes
from rene_amd.scene import Scene

NONE = 0xFFFFFFFF


# ---- the hash and the manifest ---------------------------------------------------------------------------------------------------------------------
def murmur3_32(data: bytes, seed: int = 0) -> int:
    """MurmurHash3_x86_32 as its author's reference code reads, on Python integers."""
    M = 0xFFFFFFFF
    rotl = lambda v, r: ((v << r) | (v >> (32 - r))) & M
    h = seed
    blocks = len(data) // 4
    for i in range(blocks):
        k, = struct.unpack_from("<I", data, 4 * i)
        k = rotl(k * 0xCC9E2D51 & M, 15) * 0x1B873593 & M
        h = (rotl(h ^ k, 13) * 5 + 0xE6546B64) & M
    tail, k = data[4 * blocks:], 0
    for i in reversed(range(len(tail))):
        k ^= tail[i] << (8 * i)
    if tail:
        h ^= rotl(k * 0xCC9E2D51 & M, 15) * 0x1B873593 & M
    h ^= len(data)
    h ^= h >> 16
    h = h * 0x85EBCA6B & M
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M
    return h ^ (h >> 16)


def name_hash(name) -> int:
    """The id of a name: the hash with an exponent of 0 or 255 moved off it, so that the bits are a normal float."""
    h = murmur3_32(name.encode() if isinstance(name, str) else bytes(name))
    return h ^ (1 << 23) if (h >> 23) & 255 in (0, 255) else h


def layer_key(layer_name: str) -> str:
    """The <key> of a layer's cryptomatte/<key>/* attributes: the first 7 hex digits of its name's hash."""
    return ("%08x" % name_hash(layer_name))[:7]


def manifest_of(names) -> dict:
    return {n: "%08x" % name_hash(n) for n in names}


def manifest_text(names) -> bytes:
    """The manifest's bytes: no spaces, names by their bytes, each once, " and \\ escaped, bytes below 0x20 as \\u00XX, the others copied."""
    def escaped(b: bytes) -> bytes:
        return b"".join(b"\\" + bytes([c]) if c in b'"\\' else b"\\u%04x" % c if c < 0x20 else bytes([c]) for c in b)
    return b"{" + b",".join(b'"' + escaped(n) + b'":"%08x"' % name_hash(n) for n in sorted(set(x.encode() for x in names))) + b"}"


# ---- the header ------------------------------------------------------------------------------------------------------------------------------------
def walk_header(data: bytes):
    """([(attribute name, type, value bytes), ...] in file order, the offset behind the header's terminating 0)."""
    assert struct.unpack_from("<II", data, 0) == (20000630, 2), "magic, version 2 and no flags (no long names)"
    at, attrs = 8, []
    while data[at]:
        name = data[at:data.index(b"\0", at)]
        at += len(name) + 1
        typ = data[at:data.index(b"\0", at)]
        at += len(typ) + 1
        n, = struct.unpack_from("<i", data, at)
        assert len(name) <= 31 and len(typ) <= 31
        attrs.append((name.decode(), typ.decode(), data[at + 4:at + 4 + n]))
        at += 4 + n
    return attrs, at + 1


def channel_list(value: bytes):
    """[(name, pixel type), ...] of a chlist attribute; every entry linear-less, sampled 1 x 1."""
    p, out = 0, []
    while value[p]:
        name = value[p:value.index(b"\0", p)]
        p += len(name) + 1
        typ, plinear, xs, ys = struct.unpack_from("<iiii", value, p)
        assert (plinear, xs, ys) == (0, 1, 1) and len(name) <= 31
        out.append((name.decode(), typ))
        p += 16
    assert p + 1 == len(value)
    return out


def expected_channels(layer_names):
    return sorted((f"{L}{level}.{c}" for L in layer_names for level in ("00", "01") for c in "RGBA"), key=lambda s: s.encode())


# ---- the body --------------------------------------------------------------------------------------------------------------------------------------
def ranks(rec, names):
    """One pixel's (id bits, coverage as np.float32) of ranks 0 .. 3 by the header's rules 1 to 5."""
    out = [(0, np.float32(0.0))] * 4
    n = int(rec["n"])
    if n == 0:
        return out
    merged = []  # [key, count] in slot order
    for k in range(4):
        count, i = int(rec["count"][k]), int(rec["id"][k])
        if count == 0 or i >= len(names):
            continue
        key = name_hash(names[i])
        for m in merged:
            if m[0] == key:
                m[1] = (m[1] + count) & 0xFFFFFFFF
                break
        else:
            merged.append([key, count])
    merged.sort(key=lambda m: (-m[1], m[0]))
    for r, (key, count) in enumerate(merged):
        out[r] = (key, np.float32(count) / np.float32(n))
    return out


def body(w, h, layers, records) -> bytes:
    """The uncompressed body: layers = [(layer name, ids, names), ...], records = one (h, w) array of abi.GBUFFER_DTYPE per layer."""
    order = expected_channels([L[0] for L in layers])
    planes = {name: np.zeros((h, w), np.uint32) for name in order}
    for (L, _, names), rec in zip(layers, records):
        for y in range(h):
            for x in range(w):
                rk = ranks(rec[y, x], names)
                for level, (even, odd) in (("00", (0, 1)), ("01", (2, 3))):
                    planes[f"{L}{level}.R"][y, x] = rk[even][0]
                    planes[f"{L}{level}.G"][y, x] = rk[even][1].view(np.uint32)
                    planes[f"{L}{level}.B"][y, x] = rk[odd][0]
                    planes[f"{L}{level}.A"][y, x] = rk[odd][1].view(np.uint32)
    row_bytes = w * 4 * len(order)
    return b"".join(struct.pack("<ii", y, row_bytes) + b"".join(planes[name][y].astype("<u4").tobytes() for name in order) for y in range(h))


def decode(data: bytes):
    """(w, h, {channel: (h, w) uint32 bit patterns}, attributes, compression, the offset table) of a whole file, compression 0 or 2."""
    attrs, at = walk_header(data)
    by_name = {n: v for n, _, v in attrs}
    compression = by_name["compression"][0]
    x0, y0, x1, y1 = struct.unpack("<iiii", by_name["dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    chans = channel_list(by_name["channels"])
    assert all(t == 2 for _, t in chans), "every channel is FLOAT"
    n = 4 * w * len(chans)
    table = list(struct.unpack_from(f"<{h}Q", data, at))
    out = {name: np.empty((h, w), np.uint32) for name, _ in chans}
    end = at + 8 * h
    for y in range(h):
        assert table[y] == end, "the chunks are back to back, in row order, where the table says"
        yy, size = struct.unpack_from("<ii", data, end)
        assert yy == y and 0 < size <= n
        raw = data[end + 8:end + 8 + size]
        end += 8 + size
        if size != n:
            assert compression == 2
            raw = zr.raw_from_d(np.frombuffer(zlib.decompress(raw), np.uint8))
        assert len(raw) == n
        for k, (name, _) in enumerate(chans):
            out[name][y] = np.frombuffer(raw, "<u4", w, 4 * w * k)
    assert end == len(data), "nothing behind the last chunk"
    return w, h, out, attrs, compression, table


def matte(chans, layer_name, key: int) -> np.ndarray:
    """The matte of one id as a compositor decodes it: the sum of the coverages of the ranks whose id is `key` (at most one rank per pixel)."""
    total = None
    for level in ("00", "01"):
        for i, c in (("R", "G"), ("B", "A")):
            part = np.where(chans[f"{layer_name}{level}.{i}"] == key, chans[f"{layer_name}{level}.{c}"].view(np.float32), np.float32(0.0))
            total = part if total is None else total + part
    return total


# ---- the inputs the tests share --------------------------------------------------------------------------------------------------------------------
CRAFTED_W, CRAFTED_H = 5, 3
# ids 0, 3, 6 and 7 are one name; 1 and 5 another
CRAFTED_NAMES = ["ball", "wall", "lamp", "ball", "floor", "wall", "ball", "ball"]
CRAFTED_MATERIAL_NAMES = ['say "hi"', "back\\slash", "tab\there", "plain", 'say "hi"', "m5", "m6", "m7"]


def crafted_records() -> np.ndarray:
    """5 x 3 records, one case each (the comment names it); the slots a case does not fill are the unused slot (id ~0, count 0)."""
    cases = [
        (0, 0, [], []),                                  # n == 0: a pixel no pass has filled
        (16, 14, [0, 3, 6, 7], [5, 4, 3, 2]),            # all four slots of one name: one rank of 14 / 16
        (16, 11, [0, 1, 3, 5], [4, 4, 2, 1]),            # two pairs: ball 6, wall 5
        (16, 9, [1, 2, 4], [3, 3, 3]),                   # a three-way count tie, ordered by key
        (16, 12, [1, 99, 2, NONE], [5, 4, 3, 0]),        # an id out of range is dropped
        (16, 10, [1, 2, 4, 0], [5, 0, 3, 2]),            # a zero count in the middle
        (16, 3, [2], [3]),                               # hits < n
        (16, 12, [1, 0, 3, 2], [5, 3, 3, 1]),            # the merged pair overtakes the leader
        (16, 8, [0, 1, 3], [2, 4, 2]),                   # a tie after the merge
        (3, 1, [4], [1]),                                # 1 / 3 is rounded
        (49999, 33333, [2, 4], [33333 - 7, 7]),          # a division that is not exact, a coverage near 2^-13
        (4, 4, [1, 2], [3, 3]),                          # counts beyond n (crafted): the coverages are what the division says
        (16, 6, [0, 3, 6, 1], [1, 1, 1, 3]),             # three slots merge into slot 0 and tie with the fourth
        (16, 16, [7, 5, 2, 4], [4, 4, 4, 4]),            # four names, one count: key order alone
        (0xFFFFFFFF, 5, [3, 6], [0xFFFFFFFF, 2]),        # the merged count wraps as uint32; the coverage of 2^32 - 1 samples
    ]
    rec = np.zeros((CRAFTED_H, CRAFTED_W), abi.GBUFFER_DTYPE)
    rec["id"] = NONE
    flat = rec.reshape(-1)
    for p, (n, hits, ids, counts) in enumerate(cases):
        flat[p]["n"], flat[p]["hits"] = n, hits
        flat[p]["id"][:len(ids)], flat[p]["count"][:len(counts)] = ids, counts
        flat[p]["depth_min"] = np.inf
    flat[0]["id"] = 0  # (the all-zero record)
    flat[0]["depth_min"] = 0
    return rec


def _camera(s, w, h):
    s.set_camera(glam.from_cols_array(scenes.CORNELL_WORLD_TO_CAMERA), scenes.CORNELL_FOV_DEG, w, h)


def _quad(x0, x1, y0, y1, z):
    return scenes._quad([x0, y0, z, x1, y0, z, x1, y1, z, x0, y1, z], (0.0, 0.0, 1.0))


def crafted_scene() -> Scene:
    """A 5 x 3 film over eight instances and eight materials: what a context must have to take the crafted records."""
    s = Scene.new()
    _camera(s, CRAFTED_W, CRAFTED_H)
    mats = [s.add_matte((0.5, 0.5, 0.5)) for _ in range(7)]
    light = s.add_area_light_diffuse((5.0, 5.0, 5.0))
    for k in range(8):
        s.add_sphere(0.1, mats[k % 7], area_light=light if k == 0 else 0, ctm=glam.from_translation((0.25 * k - 0.9, 1.0, 0.0)))
    assert len(s.instances) == len(CRAFTED_NAMES) and len(s.materials) == len(CRAFTED_MATERIAL_NAMES)
    return s


FILM_W, FILM_H, FRAMES = 70, 45, 16
N_CHIPS = 12


def matte_scene(w=FILM_W, h=FILM_H) -> Scene:
    """Quads and small spheres in front of the Cornell camera, the background visible around them: a wall; two quads of ONE name that overlap
    on the film; two spheres, one named; a lamp; twelve strips a twelfth of two pixels wide side by side, unnamed (object_<i>) -- more ids in one
    pixel than a record has slots.  Five materials, two of them named, one shared by the pair."""
    s = Scene.new()
    _camera(s, w, h)
    grey = s.add_matte((0.6, 0.6, 0.6), name="plaster")
    red = s.add_matte((0.6, 0.1, 0.1), name="red paint")
    blue = s.add_matte((0.1, 0.1, 0.6))
    chip = s.add_matte((0.3, 0.6, 0.3))
    dark = s.add_matte((0.0, 0.0, 0.0))
    s.add_triangle_mesh(_quad(-0.6, 0.6, 0.4, 1.6, -1.0), grey, name="wall")
    s.add_triangle_mesh(_quad(-0.5, 0.0, 0.8, 1.3, 0.0), red, name="pair")
    s.add_triangle_mesh(_quad(-0.2, 0.3, 1.0, 1.5, 0.3), red, name="pair")
    s.add_sphere(0.15, blue, ctm=glam.from_translation((0.5, 0.6, 0.2)), name="ball")
    s.add_sphere(0.1, blue, ctm=glam.from_translation((-0.7, 1.7, 0.0)))
    light = s.add_area_light_diffuse((17.0, 12.0, 4.0))
    s.add_triangle_mesh(scenes._quad([-0.2, 1.95, -0.2, 0.2, 1.95, -0.2, 0.2, 1.95, 0.2, -0.2, 1.95, 0.2], (0.0, -1.0, 0.0)), dark, area_light=light, name="lamp")
    x0, width = 0.55, 0.096 / N_CHIPS
    for k in range(N_CHIPS):
        s.add_triangle_mesh(_quad(x0 + k * width, x0 + (k + 1) * width, 1.2, 1.4, 0.5), chip)
    return s


def check_header(data, w, h, layers, compression):
    """The header of a file of layers = [(layer name, ids, names), ...], attribute by attribute; returns the offset behind it."""
    attrs, at = walk_header(data)
    names = [n for n, _, _ in attrs]
    common = ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"]
    assert names[:8] == common
    by_name = {n: (t, v) for n, t, v in attrs}
    assert by_name["compression"] == ("compression", bytes([compression]))
    assert by_name["dataWindow"] == ("box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1)) == by_name["displayWindow"]
    assert by_name["lineOrder"] == ("lineOrder", b"\0") and by_name["pixelAspectRatio"] == ("float", struct.pack("<f", 1.0))
    assert by_name["screenWindowCenter"] == ("v2f", struct.pack("<ff", 0, 0)) and by_name["screenWindowWidth"] == ("float", struct.pack("<f", 1.0))
    assert by_name["channels"][0] == "chlist"
    assert channel_list(by_name["channels"][1]) == [(c, 2) for c in expected_channels([L[0] for L in layers])]
    want = []
    for L, _, layer_names in sorted(layers, key=lambda l: l[0].encode()):
        key = layer_key(L)
        want += [f"cryptomatte/{key}/{leaf}" for leaf in ("conversion", "hash", "manifest", "name")]
        assert by_name[f"cryptomatte/{key}/conversion"] == ("string", b"uint32_to_float32")
        assert by_name[f"cryptomatte/{key}/hash"] == ("string", b"MurmurHash3_32")
        assert by_name[f"cryptomatte/{key}/name"] == ("string", L.encode())
        typ, text = by_name[f"cryptomatte/{key}/manifest"]
        assert typ == "string" and text == manifest_text(layer_names)
        assert json.loads(text.decode()) == manifest_of(layer_names)
        keys = [k.encode() for k in json.loads(text.decode(), object_pairs_hook=lambda pairs: [k for k, _ in pairs])]
        assert keys == sorted(set(n.encode() for n in layer_names)), "each distinct name once, ordered by its bytes"
    assert names[8:] == want
    return at

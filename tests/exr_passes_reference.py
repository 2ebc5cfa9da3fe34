"""Test helper (not a conftest): an independent numpy writer of the pass-layer OpenEXR file (rene_output_exr_passes, include/rene_hip.h) and the
crafted records its tests share.  The channel order comes from SORTING the name strings by their bytes, the values from the api.* reductions the
header names (occlusion_ao, occlusion_bent, bounces_depth_mean, direct_mean, indirect_mean, lights_group_mean, bounces_mean_length), the halves
from numpy's round-to-nearest-even conversion behind the clamp to the finite halves, with every NaN written as 0x7e00 as the header says."""
import struct

import numpy as np

import exr_reference
from rene_amd import abi, api

LAYERS = {"ao": abi.EXRP_AO, "bent": abi.EXRP_BENT, "bounces": abi.EXRP_BOUNCES, "direct": abi.EXRP_DIRECT, "indirect": abi.EXRP_INDIRECT,
          "lights": abi.EXRP_LIGHTS, "length": abi.EXRP_LENGTH}
OCCLUSION, DIRECT, BOUNCES, LIGHTS = (np.dtype(d) for d in (abi.OCCLUSION_DTYPE, abi.DIRECT_DTYPE, abi.BOUNCES_DTYPE, abi.LIGHTS_DTYPE))
EDGES = exr_reference.EDGE_VALUES  # above the largest half, half subnormals and the tie below the smallest, -0.0, a NaN, the infinities, ...


def written_groups(mask: int, groups: int) -> list:
    if not mask & abi.EXRP_LIGHTS:
        return []
    return [g for g in range(8) if (groups or 255) >> g & 1]


def planes(mask: int, groups: int = 0, *, occlusion=None, direct=None, bounces=None, lights=None, beauty_sum=None) -> dict:
    """{channel name: (h, w) float32} of the chosen layers, from the api's reductions."""
    out = {}
    with np.errstate(all="ignore"):
        if mask & abi.EXRP_AO:
            out["ao"] = api.occlusion_ao(occlusion)
        if mask & abi.EXRP_BENT:
            bent = api.occlusion_bent(occlusion)
            for k, c in enumerate("XYZ"):
                out[f"bent.{c}"] = bent[..., k]
        if mask & abi.EXRP_BOUNCES:
            for d in range(10):
                mean = api.bounces_depth_mean(bounces, d)
                for k, c in enumerate("RGB"):
                    out[f"depth{d}.{c}"] = mean[..., k]
        if mask & abi.EXRP_DIRECT:
            mean = api.direct_mean(direct)
            for k, c in enumerate("RGB"):
                out[f"direct.{c}"] = mean[..., k]
        if mask & abi.EXRP_INDIRECT:
            mean = api.indirect_mean(beauty_sum, direct)
            for k, c in enumerate("RGB"):
                out[f"indirect.{c}"] = mean[..., k]
        for g in written_groups(mask, groups):
            mean = api.lights_group_mean(lights, g)
            for k, c in enumerate("RGB"):
                out[f"light{g}.{c}"] = mean[..., k]
        if mask & abi.EXRP_LENGTH:
            out["pathlength"] = api.bounces_mean_length(bounces)
    return {name: np.asarray(p, np.float32) for name, p in out.items()}


def channel_order(names) -> list:
    return sorted(names, key=lambda s: s.encode())


def half_bits(v) -> np.ndarray:
    """The file's HALF of fp32 values as uint16: exr_reference.half, and 0x7e00 for every NaN."""
    v = np.asarray(v, np.float32)
    return np.where(np.isnan(v), np.uint16(0x7E00), exr_reference.half(v).view(np.uint16)).astype("<u2")


def bytes_per_pixel(mask: int, groups: int = 0) -> int:
    per = {abi.EXRP_AO: 2, abi.EXRP_BENT: 6, abi.EXRP_BOUNCES: 60, abi.EXRP_DIRECT: 6, abi.EXRP_INDIRECT: 6, abi.EXRP_LENGTH: 2}
    return sum(n for bit, n in per.items() if mask & bit) + 6 * len(written_groups(mask, groups))


def body(w: int, h: int, mask: int, groups: int = 0, **sources) -> bytes:
    p = planes(mask, groups, **sources)
    order = channel_order(p)
    bits = {name: half_bits(p[name]) for name in order}
    row_bytes = 2 * w * len(order)
    assert row_bytes == w * bytes_per_pixel(mask, groups)
    return b"".join(struct.pack("<ii", y, row_bytes) + b"".join(bits[name][y].tobytes() for name in order) for y in range(h))


def channel_names(mask: int, groups: int = 0) -> list:
    names = []
    if mask & abi.EXRP_AO:
        names.append("ao")
    if mask & abi.EXRP_BENT:
        names += [f"bent.{c}" for c in "XYZ"]
    if mask & abi.EXRP_BOUNCES:
        names += [f"depth{d}.{c}" for d in range(10) for c in "RGB"]
    if mask & abi.EXRP_DIRECT:
        names += [f"direct.{c}" for c in "RGB"]
    if mask & abi.EXRP_INDIRECT:
        names += [f"indirect.{c}" for c in "RGB"]
    names += [f"light{g}.{c}" for g in written_groups(mask, groups) for c in "RGB"]
    if mask & abi.EXRP_LENGTH:
        names.append("pathlength")
    return channel_order(names)


def light_groups_text(mask: int, groups: int, names) -> bytes:
    """The value of rene/lightGroups, b"" where no written group has a name: the manifest's shape and escaping."""
    def escaped(b):
        return b"".join(b"\\" + bytes([c]) if c in b'"\\' else b"\\u%04x" % c if c < 0x20 else bytes([c]) for c in b)
    pairs = [(g, names[g]) for g in written_groups(mask, groups) if names is not None and names[g] is not None]
    if not pairs:
        return b""
    return b"{" + b",".join(b'"light%d":"' % g + escaped(n.encode()) + b'"' for g, n in pairs) + b"}"


def _attr(name: str, typ: str, value: bytes) -> bytes:
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def attributes(w: int, h: int, mask: int, groups: int = 0, names=None, compression: int = 0) -> bytes:
    """The file from the magic through the header's terminating 0."""
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iiii", 1, 0, 1, 1) for n in channel_names(mask, groups)) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    out = struct.pack("<II", 20000630, 2) + _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([compression]))
    out += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box) + _attr("lineOrder", "lineOrder", b"\0")
    out += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + _attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
    out += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    text = light_groups_text(mask, groups, names)
    if text:
        out += _attr("rene/lightGroups", "string", text)
    return out + b"\0"


def file_bytes(w: int, h: int, mask: int, groups: int = 0, names=None, **sources) -> bytes:
    """The uncompressed file: attributes, the offset table, the body."""
    head = attributes(w, h, mask, groups, names)
    chunk = 8 + w * bytes_per_pixel(mask, groups)
    table = b"".join(struct.pack("<Q", len(head) + 8 * h + y * chunk) for y in range(h))
    return head + table + body(w, h, mask, groups, **sources)


def owned_bytes(bpp: int, owned) -> np.ndarray:
    """Boolean array over a body's bytes: those a context writes whose pixels are owned[h, w] -- the pixels' two bytes in every channel row and the
    8-byte prefix of every row that holds an owned pixel."""
    rows = []
    for y in range(owned.shape[0]):
        rows.append(np.concatenate([np.full(8, owned[y].any())] + [np.repeat(owned[y], 2)] * (bpp // 2)))
    return np.concatenate(rows)


# ---- crafted records ---------------------------------------------------------------------------------------------------------------------------
BENT_EDGES = np.array([(0, 0, 0), (0.3, -0.4, 1.2), (np.nan, 1, 2), (np.inf, 1, 2), (1, -np.inf, 2), (1e-20, 0, 0), (1e-30, 1e-30, 0), (1e30, 1, -1),
                       (-0.0, 0.0, 2.0), (-0.0, -0.0, -0.0), (3e-23, 4e-23, 0), (1e19, 1e19, 1e19), (2.0 ** -25, 0, 1), (0, 0, -5), (1e-45, 0, 0),
                       (65504.0, 65504.0, 1.0)], np.float32)


def crafted(w: int, h: int, seed: int = 7) -> dict:
    """occlusion, direct, bounces, lights (h, w) record arrays and beauty_sum (h, w, 3), noisy values salted -- pixel i of the film in row order --
    with the edges: n == 0 and rays == 0, bent_sum == 0, NaN and infinite components, sums above 65504 n, values on fp16 subnormals and on the
    tie below the smallest one, -0.0, beauty_sum < direct_sum and inf - inf."""
    rng = np.random.default_rng(seed)
    n_px = w * h
    E, nE = EDGES, len(EDGES)
    occ, dr, bn, lt = (np.zeros(n_px, d) for d in (OCCLUSION, DIRECT, BOUNCES, LIGHTS))
    f = lambda *shape: (rng.random(shape, np.float32) * np.float32(4.0)).astype(np.float32)
    # noise everywhere
    occ["rays"] = rng.integers(1, 64, n_px)
    occ["occluded"] = (occ["rays"] * rng.random(n_px)).astype(np.uint32)
    occ["hits"], occ["n"] = occ["rays"], 8
    occ["bent_sum"] = f(n_px, 3) - np.float32(2.0)
    dr["seen"], dr["distant"], dr["sampled"], dr["n"], dr["hits"] = f(n_px, 3), f(n_px, 3), f(n_px, 3), 8, 5
    beauty = (api.direct_sum(dr) + f(n_px, 3) * np.float32(3.0)).astype(np.float32)
    bn["bucket"]["sum"], bn["bucket"]["reached"] = f(n_px, 10, 3), rng.integers(0, 9, (n_px, 10))
    bn["n"], bn["length_sum"], bn["length_max"] = 8, rng.integers(8, 400, n_px), 50
    lt["group"]["sum"], lt["group"]["adds"], lt["n"], lt["lit"] = f(n_px, 8, 3), rng.integers(0, 9, (n_px, 8)), 8, 8
    for i in range(n_px):
        e3 = np.array([E[i % nE], E[(i + 7) % nE], E[(i + 14) % nE]], np.float32)
        if i < nE:  # n == 1: the edge values themselves reach the halves (x + -0 is x, -0 included)
            occ[i]["rays"], occ[i]["occluded"] = (0, 0) if i % 3 == 0 else (3, i % 4)
            dr[i]["seen"], dr[i]["distant"], dr[i]["sampled"], dr[i]["n"] = e3, -0.0, -0.0, 1
            beauty[i] = e3[::-1]
            bn[i]["n"], bn[i]["length_sum"] = 1, (0xFFFFFFFF, 0, 16777217, 3)[i % 4]
            lt[i]["n"] = 1
            for d in range(10):
                bn[i]["bucket"]["sum"][d] = np.roll(e3, d)
            for g in range(8):
                lt[i]["group"]["sum"][g] = np.roll(e3, g)[::-1]
        elif i < 2 * nE:  # n == 3: sums above 65504 n, thirds that are no halves; the indirect light is the edge value (the direct sum is -0)
            occ[i]["rays"], occ[i]["occluded"] = 16777217, (i * 1234567) % 16777217
            dr[i]["seen"], dr[i]["distant"], dr[i]["sampled"], dr[i]["n"] = -0.0, -0.0, -0.0, 1
            beauty[i] = e3
            bn[i]["n"], bn[i]["length_sum"] = 3, 65504 * 3 + i
            lt[i]["n"] = 3
            bn[i]["bucket"]["sum"][:] = np.float32(65504.0 * 3) + np.arange(30, dtype=np.float32).reshape(10, 3) * np.float32(16.0) - np.float32(200.0)
            lt[i]["group"]["sum"][:] = (e3 * np.float32(3.0))[None, :]
        elif i < 2 * nE + 8:  # the rest of the table
            k = i - 2 * nE
            if k == 0:  # n == 0 over sums that are not zero: zeros
                dr[i]["n"], bn[i]["n"], lt[i]["n"], occ[i]["rays"] = 0, 0, 0, 0
            elif k == 1:  # beauty below direct: a negative indirect
                dr[i]["seen"], dr[i]["distant"], dr[i]["sampled"], dr[i]["n"], beauty[i] = (5, 1, 9), (0.5, 0, 0), (0.25, 0, 0), 2, (2, 1, 0.5)
            elif k == 2:  # inf - inf, and inf + -inf inside the direct sum
                dr[i]["seen"], dr[i]["distant"], dr[i]["sampled"], dr[i]["n"], beauty[i] = (np.inf, np.inf, 1), (0, -np.inf, 0), (0, 0, 0), 4, (np.inf, 1, -np.inf)
            elif k == 3:  # a NaN in the radiance, a NaN in a record
                dr[i]["sampled"], beauty[i] = (np.nan, 0, 0), (1, np.nan, 2)
            elif k == 4:  # means on the half subnormals from larger counts
                bn[i]["n"] = lt[i]["n"] = dr[i]["n"] = 65536
                dr[i]["seen"], dr[i]["distant"], dr[i]["sampled"] = (2.0 ** -8, 2.0 ** -9, 3 * 2.0 ** -9), -0.0, -0.0
                beauty[i] = (2.0 ** -8 + 2.0 ** -7, 2.0 ** -9, 0)
                bn[i]["bucket"]["sum"][:] = np.float32(2.0 ** -9) * np.arange(1, 31, dtype=np.float32).reshape(10, 3)
                lt[i]["group"]["sum"][:] = np.float32(2.0 ** -10) * np.arange(1, 25, dtype=np.float32).reshape(8, 3)
            elif k == 5:
                occ[i]["rays"], occ[i]["occluded"] = 0xFFFFFFFF, 0xFFFFFFFF
            elif k == 6:
                occ[i]["rays"], occ[i]["occluded"] = 64, 64
                bn[i]["bucket"]["sum"][:] = -0.0
                lt[i]["group"]["sum"][:] = -0.0
        occ[i]["bent_sum"] = BENT_EDGES[i % len(BENT_EDGES)] if i < 3 * len(BENT_EDGES) else occ[i]["bent_sum"]
    shape = lambda a: a.reshape(h, w)
    return dict(occlusion=shape(occ), direct=shape(dr), bounces=shape(bn), lights=shape(lt), beauty_sum=beauty.reshape(h, w, 3))

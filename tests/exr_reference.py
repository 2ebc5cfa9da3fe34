"""numpy restatement of the multi-channel OpenEXR output (rene_output_exr, include/rene_hip.h): the channels of a layer mask from planes of means,
the planes of the geometry layers from rene_gbuffer's records, the file through tests/test_images.py's independent writer, and a parser of the
uncompressed scan-line files the library writes.  Everything is fp32 numpy, whose division is the correctly rounded one; the halves are numpy's
round-to-nearest-even conversion behind the clamp to the finite halves."""
import struct

import numpy as np

from rene_amd import abi
from test_images import exr_bytes

HALF_MAX = np.float32(65504.0)
# the edge values of the crafted chains: above the largest half, a half subnormal (2^-24 x 3) and the tie below the smallest one, -0.0, a NaN,
# the infinities, the largest half itself, a value that rounds up to 2^-14 and one that rounds to even
EDGE_VALUES = np.array([65505.0, 1e30, -7e4, 3 * 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -26, -0.0, np.nan, np.inf, -np.inf, 65504.0, 65519.9,
                        2.0 ** -14 * (1 - 2.0 ** -12), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-45, -1e-39, 0.0, 1.0, 0.1], np.float32)


def half(v):
    """The HALF of fp32 values: clamped to +-65504 (a NaN fails both comparisons and stays), then rounded to nearest even."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(v > HALF_MAX, HALF_MAX, np.where(v < -HALF_MAX, -HALF_MAX, v))
        return v.astype(np.float16)


def gbuffer_planes(rec):
    """The planes of the four geometry layers from an array of abi.GBUFFER_DTYPE records."""
    hits, n = rec["hits"].astype(np.float32), rec["n"].astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = np.where(rec["n"] > 0, hits / n, np.float32(0)).astype(np.float32)
        depth = np.where(rec["hits"] > 0, rec["depth_sum"] / hits, np.float32(np.inf)).astype(np.float32)
        position = np.where(rec["hits"][..., None] > 0, rec["position_sum"] / hits[..., None], np.float32(0)).astype(np.float32)
        coverage = np.where(rec["n"][..., None] > 0, rec["count"].astype(np.float32) / n[..., None], np.float32(0)).astype(np.float32)
    return dict(alpha=alpha, depth=depth, position=position, ids=rec["id"].astype(np.uint32), coverage=coverage)


_SOURCE = {"A": ("alpha", None), "B": ("beauty", 2), "G": ("beauty", 1), "R": ("beauty", 0), "P.X": ("position", 0), "P.Y": ("position", 1),
           "P.Z": ("position", 2), "Z": ("depth", None)}
for _l, _names in (("albedo", "RGB"), ("denoised", "RGB"), ("normal", "XYZ")):
    for _k, _c in enumerate(_names):
        _SOURCE[f"{_l}.{_c}"] = (_l, _k)
for _k in range(4):
    _SOURCE[f"cov{_k}"] = ("coverage", _k)
    _SOURCE[f"id{_k}"] = ("ids", _k)


def channels(mask, **planes):
    """{name: (array[h, w], type)} of the layers in `mask`, for exr_bytes."""
    out = {}
    for name, bit, typ in abi.EXR_CHANNELS:
        if not mask & bit:
            continue
        plane, k = _SOURCE[name]
        a = planes[plane] if k is None else planes[plane][..., k]
        out[name] = (half(a) if typ == "half" else np.asarray(a, {"float": np.float32, "uint": np.uint32}[typ]), typ)
    assert sorted(out) == list(out), "abi.EXR_CHANNELS is in the order of the names' bytes"
    return out


def file_bytes(mask, h, w, **planes):
    return exr_bytes(channels(mask, **planes), h, w, 0)


def parse(data):
    """(w, h, {name: array[h, w]}) of an uncompressed single-part scan-line file, every offset followed."""
    magic, version = struct.unpack_from("<II", data, 0)
    assert magic == 20000630 and version == 2
    at, attrs = 8, {}
    while data[at]:
        name = data[at:data.index(b"\0", at)]
        at += len(name) + 1
        typ = data[at:data.index(b"\0", at)]
        at += len(typ) + 1
        n, = struct.unpack_from("<i", data, at)
        attrs[name.decode()] = (typ.decode(), data[at + 4:at + 4 + n])
        at += 4 + n
    at += 1
    assert attrs["compression"][1] == b"\0" and attrs["lineOrder"][1] == b"\0"
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    chl, p, chans = attrs["channels"][1], 0, []
    while chl[p]:
        name = chl[p:chl.index(b"\0", p)]
        p += len(name) + 1
        t, = struct.unpack_from("<i", chl, p)
        p += 16
        chans.append((name.decode(), {0: "<u4", 1: "<f2", 2: "<f4"}[t]))
    out = {name: np.empty((h, w), dt) for name, dt in chans}
    for y in range(h):
        off, = struct.unpack_from("<Q", data, at + 8 * y)
        yy, size = struct.unpack_from("<ii", data, off)
        assert yy == y0 + y and size == sum(np.dtype(dt).itemsize for _, dt in chans) * w
        off += 8
        for name, dt in chans:
            out[name][y] = np.frombuffer(data, dt, w, off)
            off += np.dtype(dt).itemsize * w
    return w, h, out


def owned_bytes(mask, owned):
    """Boolean array over a body's bytes: those a context writes whose pixels are owned[h, w] -- the pixels' bytes in every channel row and the
    8-byte prefix of every row that holds an owned pixel."""
    h, w = owned.shape
    sizes = [2 if typ == "half" else 4 for _, bit, typ in abi.EXR_CHANNELS if mask & bit]
    rows = []
    for y in range(h):
        parts = [np.full(8, owned[y].any())] + [np.repeat(owned[y], s) for s in sizes]
        rows.append(np.concatenate(parts))
    return np.concatenate(rows)

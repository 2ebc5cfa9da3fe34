"""The compressed OpenEXR output (rene_exr_compress, include/rene_hip.h) restated twice, independently of the library and of each other:
(a) tail(): numpy / pure Python, the header's specification read literally -- the pre-processing, the maximal intervals of e with R div 258 full
    matches and the rest, the fixed Huffman code from RFC 1951's tables, Adler-32 from zlib -- producing the file's tail;
(b) read(): a reader that parses the attributes, follows every offset, takes size == n as a raw row and otherwise runs zlib.decompress, the
    inverse delta and the re-interleave, returning channel arrays as exr_reference.parse does.
And the crafted bodies the CPU and the GPU tests share: rows built from a wanted d, the pre-processing inverted to get raw."""
import struct
import zlib

import numpy as np

from rene_amd import abi

SEGMENT = 4096  # EXR_ZIPS_SEGMENT of kernels_exr_zips.hip, as a literal (tests/test_exr_zips_host.py holds it to the source)

# RFC 1951, section 3.2.5: length symbols 257 .. 285, their base lengths and extra bits
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]


def bytes_per_pixel(mask):
    return sum(2 if t == "half" else 4 for _, b, t in abi.EXR_CHANNELS if mask & b)


def preprocess(raw):
    """d of a row's raw bytes."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    t = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) % 256
    return d.astype(np.uint8)


def raw_from_d(d):
    """The inverse: the raw bytes whose pre-processed row is d (len(d) even)."""
    d = np.asarray(d, np.int64)
    assert d.size % 2 == 0
    steps = d - 128
    steps[0] = d[0]
    t = (np.cumsum(steps) % 256).astype(np.uint8)
    raw = np.empty(d.size, np.uint8)
    raw[0::2], raw[1::2] = t[:d.size // 2], t[d.size // 2:]
    return raw.tobytes()


class _Bits:
    def __init__(self):
        self.out, self.acc, self.cnt = bytearray(), 0, 0

    def put(self, value, n):  # LSB first
        self.acc |= value << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.cnt -= 8

    def huffman(self, code, n):  # MSB first
        self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def symbol(self, sym):
        if sym < 144:
            self.huffman(0x30 + sym, 8)
        elif sym < 256:
            self.huffman(0x190 + sym - 144, 9)
        elif sym < 280:
            self.huffman(sym - 256, 7)
        else:
            self.huffman(0xC0 + sym - 280, 8)

    def match(self, length):
        k = max(i for i, b in enumerate(_LEN_BASE) if b <= length)
        self.symbol(257 + k)
        self.put(length - _LEN_BASE[k], _LEN_EXTRA[k])
        self.huffman(1, 5)  # distance code 1: distance 2, no extra bits


def intervals(d):
    """The maximal intervals [start, end) of e == 1."""
    d = np.asarray(d, np.uint8)
    e = np.zeros(d.size + 1, bool)
    e[2:d.size] = d[2:] == d[:-2]
    edges = np.flatnonzero(e[1:] != e[:-1]) + 1
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def zlib_stream(d):
    """The stream of a pre-processed row, and how many matches it holds."""
    d = np.asarray(d, np.uint8)
    bits, at, matches = _Bits(), 0, 0
    bits.put(0x78, 8)
    bits.put(0x01, 8)
    bits.put(1, 1)  # BFINAL
    bits.put(1, 2)  # BTYPE = 01
    for start, end in intervals(d) + [(d.size, d.size)]:
        for i in range(at, start):
            bits.symbol(int(d[i]))
        run = end - start
        for _ in range(run // 258):
            bits.match(258)
        rest = run % 258
        matches += run // 258 + (rest >= 3)
        if rest >= 3:
            bits.match(rest)
        else:
            for i in range(end - rest, end):
                bits.symbol(int(d[i]))
        at = end
    bits.symbol(256)
    if bits.cnt:
        bits.put(0, 8 - bits.cnt)
    return bytes(bits.out) + struct.pack(">I", zlib.adler32(d.tobytes())), matches


def rows_of(body, w, h, mask):
    n = w * bytes_per_pixel(mask)
    body = bytes(body)
    assert len(body) == h * (8 + n)
    for y in range(h):
        at = y * (8 + n)
        assert struct.unpack_from("<ii", body, at) == (y, n)
        yield body[at + 8:at + 8 + n]


def tail(w, h, mask, body, attr_bytes, compression=2):
    """(the tail, which rows are stored raw, matches per row) of the file whose uncompressed body is `body`."""
    chunks, raw_rows, matches = [], [], []
    for y, raw in enumerate(rows_of(body, w, h, mask)):
        z, m = zlib_stream(preprocess(raw)) if compression == 2 else (raw, 0)
        stored = len(z) >= len(raw)
        data = raw if stored else z
        chunks.append(struct.pack("<ii", y, len(data)) + data)
        raw_rows.append(stored)
        matches.append(m)
    at, table = attr_bytes + 8 * h, []
    for c in chunks:
        table.append(at)
        at += len(c)
    return b"".join(struct.pack("<Q", o) for o in table) + b"".join(chunks), raw_rows, matches


def read(data):
    """(w, h, {name: array[h, w]}, compression, which rows are stored raw) of a single-part scan-line file with compression 0 or 2."""
    magic, version = struct.unpack_from("<II", data, 0)
    assert magic == 20000630 and version == 2
    at, attrs = 8, {}
    while data[at]:
        name = data[at:data.index(b"\0", at)]
        at += len(name) + 1
        typ = data[at:data.index(b"\0", at)]
        at += len(typ) + 1
        n, = struct.unpack_from("<i", data, at)
        attrs[name.decode()] = data[at + 4:at + 4 + n]
        at += 4 + n
    at += 1
    compression = attrs["compression"][0]
    assert compression in (0, 2) and attrs["lineOrder"] == b"\0"
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    chl, p, chans = attrs["channels"], 0, []
    while chl[p]:
        name = chl[p:chl.index(b"\0", p)]
        p += len(name) + 1
        chans.append((name.decode(), {0: "<u4", 1: "<f2", 2: "<f4"}[struct.unpack_from("<i", chl, p)[0]]))
        p += 16
    n = sum(np.dtype(dt).itemsize for _, dt in chans) * w
    out = {name: np.empty((h, w), dt) for name, dt in chans}
    stored, end = [], at + 8 * h
    for y in range(h):
        off, = struct.unpack_from("<Q", data, at + 8 * y)
        assert off == end, "the chunks are back to back, in row order"
        yy, size = struct.unpack_from("<ii", data, off)
        assert yy == y0 + y and 0 < size <= n
        raw = data[off + 8:off + 8 + size]
        assert len(raw) == size
        end = off + 8 + size
        stored.append(size == n)
        if size != n:
            assert compression == 2
            d = np.frombuffer(zlib.decompress(raw), np.uint8).astype(np.int64)
            assert d.size == n
            raw = raw_from_d(d)
        p = 0
        for name, dt in chans:
            out[name][y] = np.frombuffer(raw, dt, w, p)
            p += np.dtype(dt).itemsize * w
    assert end == len(data), "nothing behind the last chunk"
    return w, h, out, compression, stored


# ---- crafted bodies ------------------------------------------------------------------------------------------------------------------------------
def d_from_e(e, rng, below=256):
    """A d whose e is exactly the given 0 / 1 array (e[0] == e[1] == 0): d[i] = d[i-2] where e says so, else a byte that differs from it.
    below=144: literals of the 8-bit codes only, so that a row with a long interval is compressed, not stored raw."""
    e = np.asarray(e, bool)
    assert not e[:2].any()
    d = rng.integers(0, below, e.size).astype(np.int64)
    for i in range(2, e.size):
        if e[i]:
            d[i] = d[i - 2]
        elif d[i] == d[i - 2]:
            d[i] = (d[i] + 1 + rng.integers(0, below - 1)) % below
    return d.astype(np.uint8)


def e_with(n, spans):
    e = np.zeros(n, bool)
    for start, end in spans:
        assert 2 <= start <= end <= n
        e[start:end] = True
    return e


def body_of(rows):
    """An uncompressed body from raw rows of one length."""
    n = len(rows[0])
    assert all(len(r) == n for r in rows)
    return b"".join(struct.pack("<ii", y, n) + bytes(r) for y, r in enumerate(rows))


def alpha_case(name, ds):
    """A case from rows of wanted d: a film of ALPHA alone, two bytes per pixel."""
    ds = [np.asarray(d, np.uint8) for d in ds]
    n = ds[0].size
    return name, n // 2, len(ds), abi.EXR_ALPHA, body_of([raw_from_d(d) for d in ds])


INTERVAL_LENGTHS = [0, 1, 2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 517, 518, 519, 258 * 3 + 2, 258 * 3 + 3]


def cpu_cases():
    """(name, w, h, mask, body) of every crafted body of the CPU list."""
    rng = np.random.default_rng(20)
    cases = []
    n = 258 * 3 + 3 + 13  # 790
    cases.append(alpha_case("interval lengths", [d_from_e(e_with(n, [(5, 5 + r)]), rng) for r in INTERVAL_LENGTHS]))
    cases.append(alpha_case("two intervals a literal apart", [d_from_e(e_with(n, [(3, 3 + r), (4 + r, 4 + r + 7)]), rng) for r in (1, 2, 3, 258, 259)]))
    n = 600
    cases.append(alpha_case("interval edges", [d_from_e(e_with(n, [(2, 9)]), rng), d_from_e(e_with(n, [(2, 4)]), rng), d_from_e(e_with(n, [(n - 5, n)]), rng),
                                               d_from_e(e_with(n, [(n - 1, n)]), rng), d_from_e(e_with(n, [(n - 2, n)]), rng), d_from_e(e_with(n, [(n // 2 - 3, n // 2 + 4)]), rng),
                                               d_from_e(e_with(n, [(n // 2 - 1, n // 2 + 1)]), rng), d_from_e(e_with(n, [(2, n)]), rng),
                                               d_from_e(e_with(n, [(2, 2 + 258), (2 + 259, n)]), rng)]))
    lit = np.arange(256)
    cases.append(alpha_case("all 256 literals", [lit, lit[::-1], np.roll(lit, 77)]))
    cases.append(alpha_case("period 1 and period 2", [np.full(520, 128), np.full(520, 0), np.full(520, 255), np.resize([7, 200], 520), np.resize([143, 144], 520),
                                                      np.concatenate([[3], np.full(519, 128)])]))
    for name, w, h, mask in (("1 x 1 alpha", 1, 1, abi.EXR_ALPHA), ("3 x 2", 3, 2, abi.EXR_BEAUTY | abi.EXR_DEPTH), ("23 x 37", 23, 37, abi.EXR_ALL),
                             ("odd width 77", 77, 5, abi.EXR_BEAUTY | abi.EXR_DEPTH), ("odd width 5", 5, 9, abi.EXR_IDS)):
        n = w * bytes_per_pixel(mask)
        rows = []
        for y in range(h):  # constant, random and half-and-half rows in turn
            r = rng.integers(0, 256, n, dtype=np.uint8)
            if y % 3 == 0:
                r[:] = np.resize(rng.integers(0, 256, 4, dtype=np.uint8), n)
            elif y % 3 == 2:
                r[:n // 2] = 60
            rows.append(r.tobytes())
        cases.append((name, w, h, mask, body_of(rows)))
    n = 23 * 66
    cases.append(("random rows", 23, 6, abi.EXR_ALL, body_of([rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(6)])))
    cases.append(("constant rows", 23, 6, abi.EXR_ALL, body_of([np.resize(rng.integers(0, 256, 4, dtype=np.uint8), n).tobytes() for _ in range(6)])))
    cases.append(("mixed rows", 23, 6, abi.EXR_ALL, body_of([(rng.integers(0, 256, n, dtype=np.uint8) if y % 2 else np.full(n, 9 * y, np.uint8)).tobytes() for y in range(6)])))
    return cases


def segment_cases():
    """The bodies that aim at the kernels' segment edges.  A row's n = W x bytes_per_pixel is even, so the rows next to a segment's length are
    SEGMENT - 2 and SEGMENT + 2 bytes; the odd positions on either side of an edge are reached by the intervals, which start and end at every
    edge - 2 .. edge + 2.  Every row but the marked ones has literals of 8 bits and an interval of 700 positions near its start, so that it
    is compressed and the encode kernel writes its bits."""
    rng = np.random.default_rng(21)
    cases = []
    first = (10, 710)
    row = lambda n, spans: d_from_e(e_with(n, [first] + spans), rng, 144)
    for n in (SEGMENT - 2, SEGMENT, SEGMENT + 2):
        cases.append(alpha_case(f"rows of {n} bytes", [row(n, [(n - 300, n)]), row(n, []), row(n, [(712, n)]), row(n, [(n - 2, n)]), row(n, [(n - 1, n)]),
                                                      row(n, [(n - 258, n)]), row(n, [(n - 259, n)]), rng.integers(0, 256, n)]))  # (the last one: stored raw)
    n = 3 * SEGMENT + 700
    edges = (SEGMENT, 2 * SEGMENT, 3 * SEGMENT)
    rows = []
    for delta in range(-2, 3):
        rows.append(row(n, [(e + delta - 300, e + delta) for e in edges]))  # ending at the edge
        rows.append(row(n, [(e + delta, e + delta + 300) for e in edges]))  # starting at it, longer than the look-ahead
        rows.append(row(n, [(e + delta, e + delta + 3 + k) for k, e in enumerate(edges)]))  # short ones
        rows.append(row(n, [(e + delta - 1, e + delta + 1) for e in edges]))  # two positions across it: literals
        rows.append(row(n, [(e + delta, e + delta + 258 + k) for k, e in enumerate(edges)]))  # ending where the look-ahead does
        rows.append(row(n, [(e + delta - 258, e + delta + 258 + 2) for e in edges]))  # a full match on either side, a rest of two
    rows.append(row(n, [(712, n - 10)]))  # one interval over every segment
    rows.append(d_from_e(e_with(n, [(2, n)]), rng))
    rows.append(d_from_e(e_with(n, []), rng))  # literals only (stored raw)
    cases.append(alpha_case("intervals at every segment edge", rows))
    return cases

"""The render-state format (include/rene_hip.h, the checkpoint's section) restated in numpy from its text alone: build a part, parse a part,
a tile's checksum.  Nothing here calls the library.

A part: a 256-byte header, 32 bytes per tile in ascending tile order, then per tile 294912 bytes of payload,
float32 [8 chains][3 layers][32 dy][32 dx][3], pixels row-major inside the tile, zero outside the image.  Little-endian throughout."""
import numpy as np

MAGIC = 0x54534E52
VERSION = 1
HEADER_BYTES = 256
TILE = 32
TILE_BYTES = 8 * 3 * TILE * TILE * 3 * 4
TILE_DWORDS = TILE_BYTES // 4
ACTIVE = 1

HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("header_bytes", "<u4"), ("tile_size", "<u4"), ("width", "<u4"), ("height", "<u4"),
                         ("tiles_x", "<u4"), ("tiles_y", "<u4"), ("seed", "<u4"), ("frame_base", "<u4"), ("n_frames", "<u4"),
                         ("frames_contiguous", "<u4"), ("loaded", "<u4"), ("n_tiles", "<u4"), ("paths", "<u8"), ("chain_frames", "<u8", (8,)),
                         ("fingerprint", "<u8", (2,)), ("payload_offset", "<u8"), ("total_bytes", "<u8"), ("reserved", "u1", (96,))])
TILE_DTYPE = np.dtype([("tile", "<u4"), ("n_frames", "<u4"), ("flags", "<u4"), ("c0", "<u4"), ("c1", "<u4"), ("reserved", "<u4", (3,))])
assert HEADER_DTYPE.itemsize == HEADER_BYTES and TILE_DTYPE.itemsize == 32 and TILE_BYTES == 294912


def grid(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def checksum(dwords):
    """c0 = sum w_i, c1 = sum (i + 1) w_i over a tile's payload dwords in payload order, both mod 2^32 -- with Python integers."""
    c0 = c1 = 0
    for i, w in enumerate(np.asarray(dwords, np.uint32).reshape(-1).tolist()):
        c0 += w
        c1 += (i + 1) * w
    return c0 & 0xFFFFFFFF, c1 & 0xFFFFFFFF


def checksum_fast(dwords):
    """The same two sums in uint64 numpy arithmetic (wrap-around is the modulus's multiple), for whole states."""
    w = np.asarray(dwords, np.uint32).reshape(-1).astype(np.uint64)
    i = np.arange(1, w.size + 1, dtype=np.uint64)
    return int(w.sum() & np.uint64(0xFFFFFFFF)), int((w * i).sum() & np.uint64(0xFFFFFFFF))


def chain_frames(first_frame, n):
    """frame f belongs to chain f % 8"""
    out = [0] * 8
    for f in range(first_frame, first_frame + n):
        out[f % 8] += 1
    return out


def tile_payload(chains_u32, tile, width, height):
    """One tile's payload from chains (8, 3, H, W, 3) as uint32 bits: [8][3][32][32][3], zero outside the image."""
    tx, _ = grid(width, height)
    x0, y0 = (tile % tx) * TILE, (tile // tx) * TILE
    out = np.zeros((8, 3, TILE, TILE, 3), np.uint32)
    h, w = min(TILE, height - y0), min(TILE, width - x0)
    out[:, :, :h, :w, :] = chains_u32[:, :, y0:y0 + h, x0:x0 + w, :]
    return out


def build(chains, width, height, seed, frame_base, tile_frames, active, fingerprint, tiles=None, loaded=0, paths=0, frames_contiguous=1, n_frames=None):
    """A part as a uint8 array.  chains: (8, 3, H, W, 3) float32 (or uint32 bits); tile_frames / active: per tile of the full grid, row-major;
    tiles: the grid tiles in the part, ascending (default: all)."""
    c = np.ascontiguousarray(chains)
    c = c.view(np.uint32) if c.dtype == np.float32 else c.astype(np.uint32)
    tx, ty = grid(width, height)
    tiles = list(range(tx * ty)) if tiles is None else list(tiles)
    tf = np.asarray(tile_frames, np.uint32).reshape(-1)
    act = np.asarray(active).reshape(-1)
    n = int(max([int(tf[t]) for t in tiles], default=0)) if n_frames is None else n_frames
    h = np.zeros(1, HEADER_DTYPE)
    h["magic"], h["version"], h["header_bytes"], h["tile_size"] = MAGIC, VERSION, HEADER_BYTES, TILE
    h["width"], h["height"], h["tiles_x"], h["tiles_y"] = width, height, tx, ty
    h["seed"], h["frame_base"], h["n_frames"], h["frames_contiguous"], h["loaded"], h["n_tiles"] = seed, frame_base, n, frames_contiguous, loaded, len(tiles)
    h["paths"] = paths
    h["chain_frames"][0] = chain_frames(frame_base, n)
    h["fingerprint"][0] = fingerprint
    h["payload_offset"] = HEADER_BYTES + 32 * len(tiles)
    h["total_bytes"] = HEADER_BYTES + (32 + TILE_BYTES) * len(tiles)
    table = np.zeros(len(tiles), TILE_DTYPE)
    payloads = []
    for i, t in enumerate(tiles):
        p = tile_payload(c, t, width, height)
        table[i]["tile"], table[i]["n_frames"], table[i]["flags"] = t, tf[t], ACTIVE if act[t] else 0
        table[i]["c0"], table[i]["c1"] = checksum_fast(p)
        payloads.append(p.reshape(-1).view(np.uint8))
    return np.concatenate([h.view(np.uint8).reshape(-1), table.view(np.uint8).reshape(-1)] + payloads)


def parse(blob):
    """(header record, tile table, payload (n_tiles, 8, 3, 32, 32, 3) uint32) of a part."""
    b = np.ascontiguousarray(np.asarray(blob, np.uint8))
    h = b[:HEADER_BYTES].view(HEADER_DTYPE)[0]
    n = int(h["n_tiles"])
    table = b[HEADER_BYTES:HEADER_BYTES + 32 * n].view(TILE_DTYPE)
    off = int(h["payload_offset"])
    payload = b[off:off + n * TILE_BYTES].view(np.uint32).reshape(n, 8, 3, TILE, TILE, 3)
    return h, table, payload


def chains_of(blob, width, height):
    """The part's payload put back on the film: (8, 3, H, W, 3) uint32 (tiles not in the part: zero)."""
    h, table, payload = parse(blob)
    tx, _ = grid(width, height)
    out = np.zeros((8, 3, height, width, 3), np.uint32)
    for i, t in enumerate(table["tile"].tolist()):
        x0, y0 = (t % tx) * TILE, (t // tx) * TILE
        hh, ww = min(TILE, height - y0), min(TILE, width - x0)
        out[:, :, y0:y0 + hh, x0:x0 + ww, :] = payload[i, :, :, :hh, :ww, :]
    return out

"""The render-state format's host side (include/rene_hip.h, the checkpoint's section), without a GPU: rene_state_inspect, rene_state_tiles,
rene_state_verify and rene_state_bytes against parts that tests/state_reference.py builds in numpy from the format text alone; the checksum
against Python integers; rene_scene_fingerprint."""
import numpy as np
import pytest

import state_reference as sr
from rene_amd import abi, api, scenes

W, H = 70, 45                      # 3 x 2 tiles, ragged both ways
TILE_FRAMES = [21, 13, 21, 0, 21, 8]  # uneven, one tile without frames
ACTIVE = [1, 0, 1, 0, 1, 0]           # the active tiles hold N = 21
FINGERPRINT = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
SEED, FRAME_BASE, PATHS = 0xC0FFEE, 100003, 12345678901


@pytest.fixture(scope="module")
def part(hip_lib):
    rng = np.random.default_rng(11)
    chains = rng.integers(0, 2 ** 32, (8, 3, H, W, 3), dtype=np.uint64).astype(np.uint32)  # any bits: NaNs, denormals, -0.0 among them
    blob = sr.build(chains, W, H, SEED, FRAME_BASE, TILE_FRAMES, ACTIVE, FINGERPRINT, paths=PATHS)
    return chains, blob


def _refused(call, blob, *words):
    with pytest.raises(api.ReneError) as e:
        call(blob)
    assert e.value.code == -1, e.value  # RENE_ERR_INVALID_ARGUMENT
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def test_a_part_built_from_the_format_text_is_accepted_and_read_back(part):
    chains, blob = part
    assert api.state_bytes(W, H) == blob.size == 256 + 6 * (32 + 294912)
    info = api.state_info(blob).as_dict()
    want = dict(version=1, width=W, height=H, tile_size=32, tiles_x=3, tiles_y=2, seed=SEED, frame_base=FRAME_BASE, n_frames=21, frames_contiguous=1,
                loaded=0, n_tiles=6, paths=PATHS, chain_frames=sr.chain_frames(FRAME_BASE, 21), fingerprint=FINGERPRINT, payload_offset=256 + 6 * 32,
                total_bytes=blob.size)
    assert {k: info[k] for k in want} == want
    t = api.state_tiles(blob)
    assert t["tile"].tolist() == list(range(6)) and t["n_frames"].tolist() == TILE_FRAMES and t["flags"].tolist() == ACTIVE
    _, table, payload = sr.parse(blob)
    assert t["c0"].tolist() == table["c0"].tolist() and t["c1"].tolist() == table["c1"].tolist()
    api.state_verify(blob)
    # the payload is row-major inside the tile and zero outside the image
    np.testing.assert_array_equal(sr.chains_of(blob, W, H), chains)
    assert not payload[2, :, :, :, W - 64:, :].any() and not payload[5, :, :, H - 32:, :, :].any()
    # a shard's part: the tiles 1, 3, 5 of the grid
    shard = sr.build(chains, W, H, SEED, FRAME_BASE, TILE_FRAMES, ACTIVE, FINGERPRINT, tiles=[1, 3, 5], n_frames=13)
    assert api.state_bytes(W, H, 1, 2) == shard.size
    assert api.state_tiles(shard)["tile"].tolist() == [1, 3, 5] and api.state_info(shard).n_frames == 13
    assert api.state_bytes(W, H, 2, 2) == 0 and api.state_bytes(0, H) == 0


@pytest.mark.parametrize("cut, what", [(100, "header"), (256, "tile table"), (256 + 3 * 32 + 5, "tile table"),
                                       (256 + 6 * 32 + 2 * 294912 + 1000, "payload of the part's tile #2"), (-1, "payload of the part's tile #5")])
def test_truncation_is_named(part, cut, what):
    _, blob = part
    short = blob[:cut].copy()
    for call in (api.state_info, api.state_tiles, api.state_verify):
        _refused(call, short, "truncated", what)


def test_one_flipped_payload_bit_is_found_by_verify_which_names_the_tile(part):
    _, blob = part
    bad = blob.copy()
    bad[256 + 6 * 32 + 4 * 294912 + 77777] ^= 0x10  # inside tile 4's payload
    api.state_info(bad)  # the header and the table are still consistent
    _refused(api.state_verify, bad, "checksum mismatch in tile 4")


def test_table_defects_are_named(part):
    _, blob = part
    table = slice(256, 256 + 6 * 32)

    def with_table(edit):
        b = blob.copy()
        t = b[table].view(sr.TILE_DTYPE)
        edit(t)
        return b

    def swap(t):
        t[[1, 2]] = t[[2, 1]]

    def dup(t):
        t[3] = t[2]

    def below(t):
        t[1]["flags"] = 1  # N_t = 13 < N = 21

    for call in (api.state_info, api.state_tiles, api.state_verify):
        _refused(call, with_table(swap), "out of order")
        _refused(call, with_table(dup), "duplicate tile 2")
        _refused(call, with_table(below), "active tile 1", "below")
    bad_magic = blob.copy()
    bad_magic[0] ^= 1
    _refused(api.state_info, bad_magic, "magic")
    reserved = blob.copy()
    reserved[200] = 1
    _refused(api.state_info, reserved, "reserved")


def test_checksum_against_python_integers(hip_lib):
    """c0 = sum w_i, c1 = sum (i + 1) w_i mod 2^32 over the 73728 payload dwords, on three literal payloads."""
    n = sr.TILE_DWORDS
    assert n == 73728
    literals = [np.zeros(n, np.uint32),
                np.full(n, 0xFFFFFFFF, np.uint32),
                ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % 2 ** 32).astype(np.uint32)]
    # the second by hand: sum of -1 over n dwords, and -n (n + 1) / 2
    assert sr.checksum(literals[1]) == ((-n) % 2 ** 32, (-(n * (n + 1) // 2)) % 2 ** 32)
    for w in literals:
        c0, c1 = sr.checksum(w)  # Python integers
        assert (c0, c1) == sr.checksum_fast(w)
        chains = w.reshape(8, 3, 32, 32, 3)  # a 32 x 32 film: the one tile's payload is the chains as they are
        blob = sr.build(chains, 32, 32, 1, 0, [8], [1], FINGERPRINT)
        t = blob[256:288].view(sr.TILE_DTYPE)
        t["c0"], t["c1"] = c0, c1
        api.state_verify(blob)
        assert (int(api.state_tiles(blob)["c0"][0]), int(api.state_tiles(blob)["c1"][0])) == (c0, c1)
        for field in ("c0", "c1"):
            off = blob.copy()
            ot = off[256:288].view(sr.TILE_DTYPE)
            ot[field] = (int(ot[field][0]) + 1) % 2 ** 32
            _refused(api.state_verify, off, "checksum mismatch in tile 0")
    # c1 weighs the position: the same dwords in another order keep c0 and change c1
    swapped = literals[2].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert sr.checksum(swapped)[0] == sr.checksum(literals[2])[0] and sr.checksum(swapped)[1] != sr.checksum(literals[2])[1]


def test_scene_fingerprint(hip_lib):
    base = api.scene_fingerprint(scenes.cornell_box(64, 64))
    assert base == api.scene_fingerprint(scenes.cornell_box(64, 64))  # two builds of the same scene
    assert all(0 <= v < 2 ** 64 for v in base) and base[0] != base[1]
    s = scenes.cornell_box(64, 64)
    v = np.array(s.meshes[0].vertices, dtype=np.float32, copy=True)
    v.view(np.uint32)[1, 2] ^= 1  # one bit of one vertex
    s.meshes[0].vertices = v
    one_bit = api.scene_fingerprint(s)
    s = scenes.cornell_box(64, 64)
    s.camera_to_world = np.array(s.camera_to_world, copy=True)
    s.camera_to_world[1, 3] = np.nextafter(np.float32(s.camera_to_world[1, 3]), np.float32(np.inf))  # one camera float
    camera = api.scene_fingerprint(s)
    xres = api.scene_fingerprint(scenes.cornell_box(65, 64))
    prints = [base, one_bit, camera, xres]
    for i in range(4):
        for j in range(i):
            assert prints[i][0] != prints[j][0] and prints[i][1] != prints[j][1], (i, j)
    assert api.scene_fingerprint(scenes.cornell_box(64, 64).to_desc()) == base  # a packed scene as well

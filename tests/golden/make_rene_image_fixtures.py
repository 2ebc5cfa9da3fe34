"""Box-filtered copies of rene's OWN published renders (images/cornell-box.png 1024x1024,
images/veach-mis.png 1280x720; README.md:27-59 of the reference, produced by its Vulkan path at
5000 spp) as small golden fixtures for the T2 parity tier.  These are output
data of the reference, not source.  The teapot / teapot-full images are OIDN-denoised, and the teapot scene's environment
map is missing from the checkout: their RADIANCE is not used.  The teapot image's GEOMETRY is (tier T3, tests/t3_geometry.py):
which pixels are brighter than the floor's dark squares -- the checkerboard's phase and the teapot's outline.  The dragon
scene cannot be loaded here (missing meshes).

  rene_<scene>_box8.npy   8 x 8 means of the sRGB values (f32): the round-1 T2 fixtures
  rene_<scene>_box4.npy   [2][H/4][W/4][3] f16: 4 x 4 means of the sRGB values, and 4 x 4 means of the values decoded to
                          linear light (inverse of main.rs:1768-1774) -- the region-wise energy checks of tests/t2_regions.py

  rene_dragon_box4.npy    [2][180][320] f16: images/dragon.png (1280 x 720, NOT denoised: README.md:37-43), channel mean, 4 x 4 means of the sRGB
                          values and of the values decoded to linear light -- the lit surfaces of the 12 meshes the checkout holds
                          (tests/t2_regions.py, dragon_lit_ratio)
  tungsten_cornell_box8.npy  sample_scenes/cornell-box/TungstenRender.png (1024 x 1024, the unbiased Tungsten render shipped with
                          the scene; data, not source) as 8 x 8 means of the sRGB values (f32): the second yardstick of the T2 Cornell test
  sample_scenes/<scene>/TungstenRender_rows512-639.{exr,png}   rows 512 - 639 of sample_scenes/<scene>/TungstenRender.{exr,png}
                          (cornell-box, veach-mis): real PIZ files for the EXR decoder's test at a tenth of the size.  The EXR keeps
                          four of the file's 32-line PIZ chunks byte for byte (only the header's windows, the offset table and each
                          chunk's y change; nothing is re-encoded); the PNG is the same rows of the companion render, losslessly
  rene_teapot_bright.npy  images/teapot.png (1280 x 720) as ONE bit per pixel, np.packbits of  luminance > 0.51  row by row
                          (Rec. 709 luminance of the sRGB values; the dark squares of the floor end at 0.487, its light squares begin at 0.628)

    python tests/golden/make_rene_image_fixtures.py      # needs /root/reference
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/images"
SCENES = os.path.join(os.path.dirname(REF), "sample_scenes")


def load(path):
    return np.asarray(Image.open(path).convert("RGB"), np.float32) / 255.0


def box(a, k):
    h, w, _ = a.shape
    return a[: h // k * k, : w // k * k].reshape(h // k, k, w // k, k, 3).mean(axis=(1, 3)).astype(np.float32)


def box1(a, k):  # one channel
    h, w, _ = a.shape
    return a.reshape(h // k, k, w // k, k).mean(axis=(1, 3)).astype(np.float32)


def to_linear(s):  # inverse of gamma_correct, main.rs:1768-1774
    return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4).astype(np.float32)


TEAPOT_BRIGHT = 0.51
PIZ_BAND = (16, 4)  # first PIZ chunk, chunks: rows 512 - 639, the middle of both renders


def exr_rows(src: bytes, first_block: int, n_blocks: int) -> bytes:
    """A single-part scanline PIZ file (32 lines per chunk) cut to its chunks first_block .. first_block + n_blocks - 1, their
    compressed bytes unchanged: the data and display windows become rows 0 .. 32 n_blocks - 1, each chunk's y moves up to match."""
    import struct
    assert struct.unpack("<ii", src[:8]) == (20000630, 2)  # magic, version 2: single part, scan lines
    p, out, width_height = 8, bytearray(src[:8]), None
    while src[p] != 0:  # attributes: name \0 type \0 size value
        e = src.index(b"\0", p)
        e2 = src.index(b"\0", e + 1)
        name, (n,) = src[p:e], struct.unpack("<i", src[e2 + 1:e2 + 5])
        v = src[e2 + 5:e2 + 5 + n]
        if name == b"compression":
            assert v == b"\x04", "PIZ only"
        if name in (b"dataWindow", b"displayWindow"):
            x0, y0, x1, y1 = struct.unpack("<4i", v)
            assert y0 == 0
            width_height = width_height or (x1 - x0 + 1, y1 + 1)
            v = struct.pack("<4i", x0, 0, x1, 32 * n_blocks - 1)
        out += src[p:e2 + 1] + struct.pack("<i", len(v)) + v
        p = e2 + 5 + n
    out += b"\0"
    p += 1
    n_all = (width_height[1] + 31) // 32
    offsets = struct.unpack(f"<{n_all}Q", src[p:p + 8 * n_all])
    assert first_block + n_blocks <= n_all and 32 * (first_block + n_blocks) <= width_height[1]
    chunks = []
    for k in range(first_block, first_block + n_blocks):
        y, size = struct.unpack("<ii", src[offsets[k]:offsets[k] + 8])
        assert y == 32 * k
        chunks.append(struct.pack("<ii", y - 32 * first_block, size) + src[offsets[k] + 8:offsets[k] + 8 + size])
    at, table = len(out) + 8 * n_blocks, []
    for c in chunks:
        table.append(at)
        at += len(c)
    return bytes(out) + struct.pack(f"<{n_blocks}Q", *table) + b"".join(chunks)


def teapot_bright(path=os.path.join(REF, "teapot.png")):
    """[720][1280] bool: rene's teapot render brighter than the floor's dark squares."""
    a = load(path)
    return (a @ np.array([0.2126, 0.7152, 0.0722], np.float32)) > TEAPOT_BRIGHT


if __name__ == "__main__":
    d = load(os.path.join(REF, "dragon.png")).mean(axis=2, keepdims=True)
    np.save(os.path.join(HERE, "rene_dragon_box4.npy"), np.stack([box1(d, 4), box1(to_linear(d), 4)]).astype(np.float16))
    np.save(os.path.join(HERE, "rene_teapot_bright.npy"), np.packbits(teapot_bright(), axis=1))  # [720][160] u8
    np.save(os.path.join(HERE, "tungsten_cornell_box8.npy"), box(load(os.path.join(SCENES, "cornell-box", "TungstenRender.png")), 8))  # 128x128x3
    k0, nb = PIZ_BAND
    for scene in ("cornell-box", "veach-mis"):
        src, dst = os.path.join(SCENES, scene, "TungstenRender"), os.path.join(HERE, "sample_scenes", scene, "TungstenRender_rows512-639")
        open(dst + ".exr", "wb").write(exr_rows(open(src + ".exr", "rb").read(), k0, nb))
        Image.fromarray(np.asarray(Image.open(src + ".png"))[32 * k0:32 * (k0 + nb)]).save(dst + ".png")
    for name, png in (("cornell", "cornell-box.png"), ("veach_mis", "veach-mis.png")):
        a = load(os.path.join(REF, png))
        np.save(os.path.join(HERE, f"rene_{name}_box8.npy"), box(a, 8))                    # 128x128x3 / 90x160x3
        np.save(os.path.join(HERE, f"rene_{name}_box4.npy"), np.stack([box(a, 4), box(to_linear(a), 4)]).astype(np.float16))

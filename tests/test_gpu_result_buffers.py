"""GPU: the library-owned results -- the feature tensor, the 8-bit image, the geometry records, a shard's packed denoiser buffer -- through the
code they share (Result, result_buffer, result_download, check_device_destination in rene_hip.cpp): the exact words and codes of the refusals
that need a context, what rene_reset invalidates and what it leaves, and the downloads -- straight and through the pinned staging, across its
piece boundary -- against the device path, which shares nothing with them.  tests/test_result_buffers_host.py has the refusals that need no context."""
import ctypes as C

import numpy as np
import pytest

from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48
GETTERS = ("rene_features_buffer", "rene_output_buffer", "rene_gbuffer_buffer", "rene_denoise_shard_buffer")
DOWNLOADS = ("rene_download_features", "rene_download_output", "rene_download_gbuffer", "rene_download_denoise_shard")
NO_FEATURES = "no rene_export_features into the library's buffer since the context was created or reset"
NO_OUTPUT = "no rene_output_8bit into the library's buffer since the context was created or reset"
NO_GBUFFER = "no rene_gbuffer into the library's buffer since the context was created"
NO_SHARD = "no rene_denoise_shard_prepare since the context was created or reset"
NONE = dict(zip(GETTERS + DOWNLOADS, (NO_FEATURES, NO_OUTPUT, NO_GBUFFER, NO_SHARD) * 2))
TOO_SMALL = {"rene_download_features": "destination too small", "rene_download_output": "destination too small",
             "rene_download_gbuffer": "destination too small", "rene_download_denoise_shard": "dst_bytes is smaller than the packed buffer"}
IMAGE_BYTES = "height x width x bytes per pixel"
# the destination calls: what dst_bytes is compared with, the alignment and its wording, the bytes of the default parameters' result on the W x H film
DESTINATIONS = {
    "rene_export_features": ("channels x height x width x element size", 4, "aligned to its element size", W * H * 9 * 4, api.feature_params_default),
    "rene_output_8bit": (IMAGE_BYTES, 4, "4-byte aligned", W * H * 3, api.output_params_default),
    "rene_gbuffer": (IMAGE_BYTES, 16, "16-byte aligned", W * H * 64, api.gbuffer_params_default),
}


def refused(rc, text):
    got = api.lib().rene_last_error().decode()
    assert rc == -1 and got == text, (rc, got)  # -1: RENE_ERR_INVALID_ARGUMENT


def get(r, fn, ptr=True, n=True):
    p, size = C.c_void_p(), C.c_size_t()
    rc = getattr(api.lib(), fn)(r._h, C.byref(p) if ptr else None, C.byref(size) if n else None)
    return rc, p.value, size.value


def download(r, fn, n_bytes):
    dst = np.full(max(n_bytes, 1), 0xAB, np.uint8)
    return getattr(api.lib(), fn)(r._h, dst.ctypes.data_as(C.c_void_p), n_bytes), dst


def device_bytes(ptr, n):
    """The n bytes at a device pointer, read by torch: a tensor over the memory as it is (the CUDA array interface), copied to the host."""
    import torch

    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(View(), device="cuda").cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        yield r


def produce(r):
    r.render(0, 8)
    r.features()
    r.rgb8()
    r.gbuffer()
    r.denoise_shard_prepare()  # (an unsharded context is a shard of one)


def test_no_result_before_a_producing_call_and_after_reset(ctx):
    r = ctx
    for fn in GETTERS:
        refused(get(r, fn)[0], f"{fn}: {NONE[fn]}")
    for fn in DOWNLOADS:
        rc, dst = download(r, fn, 1 << 16)
        refused(rc, f"{fn}: {NONE[fn]}")
        assert (dst == 0xAB).all()
    produce(r)
    sizes = {}
    for fn, dl in zip(GETTERS, DOWNLOADS):
        rc, ptr, n = get(r, fn)
        assert rc == 0 and ptr and n, fn
        sizes[dl] = n
        refused(get(r, fn, ptr=False)[0], f"{fn}: NULL argument")
        if fn == "rene_denoise_shard_buffer":  # the one getter that may be asked for the pointer alone
            assert get(r, fn, n=False)[:2] == (0, ptr)
        else:
            refused(get(r, fn, n=False)[0], f"{fn}: NULL argument")
        rc, dst = download(r, dl, n - 1)
        refused(rc, f"{dl}: {TOO_SMALL[dl]}")
        assert (dst == 0xAB).all()
        refused(getattr(api.lib(), dl)(r._h, None, n), f"{dl}: NULL argument")
        rc, dst = download(r, dl, n)
        assert rc == 0 and np.array_equal(dst, device_bytes(ptr, n)), dl
    assert sizes == {"rene_download_features": W * H * 9 * 4, "rene_download_output": W * H * 3, "rene_download_gbuffer": W * H * 64,
                     "rene_download_denoise_shard": api.denoise_shard_bytes(W, H)}
    records = (get(r, "rene_gbuffer_buffer"), download(r, "rene_download_gbuffer", W * H * 64)[1])
    r.reset()
    for fn in GETTERS + DOWNLOADS:
        if "gbuffer" in fn:
            continue
        rc = get(r, fn)[0] if fn in GETTERS else download(r, fn, 1 << 16)[0]
        refused(rc, f"{fn}: {NONE[fn]}")
    # the geometry pass reads no frame of the context's: its result outlives the reset
    assert get(r, "rene_gbuffer_buffer") == records[0]
    rc, dst = download(r, "rene_download_gbuffer", W * H * 64)
    assert rc == 0 and np.array_equal(dst, records[1]) and np.array_equal(dst, device_bytes(*records[0][1:]))


def destination_call(r, fn, tensor_ptr, n_bytes):
    return getattr(api.lib(), fn)(r._h, C.byref(DESTINATIONS[fn][4]()), C.c_void_p(tensor_ptr), n_bytes)


@pytest.mark.parametrize("fn", DESTINATIONS)
def test_a_bad_destination_is_refused_in_the_calls_own_words(ctx, fn):
    import torch
    r = ctx
    r.reset()
    r.render(0, 8)
    size_is, align, align_is, need, _ = DESTINATIONS[fn]
    t = torch.full((need + 32,), 0xAB, dtype=torch.uint8, device="cuda")  # (room behind a misaligned pointer)
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    refused(destination_call(r, fn, t.data_ptr(), need - 1), f"{fn}: dst_bytes is smaller than {size_is}")
    refused(destination_call(r, fn, t.data_ptr() + align // 2, need), f"{fn}: the destination is not {align_is}")
    pinned = torch.full((need,), 0xAB, dtype=torch.uint8).pin_memory()
    refused(destination_call(r, fn, pinned.data_ptr(), need), f"{fn}: the destination is not device memory")
    r.sync()
    assert (t == 0xAB).all().item() and (pinned == 0xAB).all().item()  # nothing was launched on either
    assert destination_call(r, fn, t.data_ptr(), need) == 0
    r.sync()
    got = t.cpu().numpy()
    assert (got[need:] == 0xAB).all()
    want = {"rene_export_features": r.features, "rene_output_8bit": r.rgb8, "rene_gbuffer": r.gbuffer}[fn]()
    assert got[:need].tobytes() == want.tobytes()


@pytest.mark.parametrize("fn", DESTINATIONS)
def test_a_destination_on_another_device(ctx, fn):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    need = DESTINATIONS[fn][3]
    t = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda:1")
    torch.cuda.synchronize(1)
    refused(destination_call(ctx, fn, t.data_ptr(), need), f"{fn}: the destination is on another device than the context")
    assert (t == 0xAB).all().item()


def test_downloads_across_a_staging_piece_equal_the_device_path():
    """416 x 300, the full feature mask in fp32: 17 x 124 800 x 4 B = 8 486 400 B, more than 8 MiB (the piece of the staged copy) by a tail of 97 792 B.
    The tensor is copied straight into the caller's memory; the image and the records of the film go through the staging."""
    import torch
    w, h = 416, 300
    assert 17 * w * h * 4 == (8 << 20) + 97792
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.render(0, 4)
        got = r.features(abi.FEATURE_ALL, "f32", "chw")
        t = r.features_into(torch.full((17, h, w), -7.0, device="cuda"), abi.FEATURE_ALL, "chw")
        r.sync()
        assert got.any() and got.tobytes() == t.cpu().numpy().tobytes()
        ptr, n = r.features_buffer()
        assert n == got.nbytes and got.tobytes() == device_bytes(ptr, n).tobytes()
        got = r.rgb8(alpha=True)
        t = r.rgb8_into(torch.full((h, w, 4), 0xAB, dtype=torch.uint8, device="cuda"), alpha=True)
        r.sync()
        assert got.any() and got.tobytes() == t.cpu().numpy().tobytes()
        got = r.gbuffer()
        t = r.gbuffer_into(torch.full((h * w * 64,), 0xAB, dtype=torch.uint8, device="cuda"))
        r.sync()
        assert (got["n"] == 16).all() and got.tobytes() == t.cpu().numpy().tobytes()


def test_the_staged_copy_across_its_pieces_equals_the_device_path():
    """The two results that are downloaded through the pinned staging, on a film that makes them longer than its 8 MiB piece: 1449 x 1449 with
    alpha is 8 398 404 B, one piece and a tail of 9 796 B, which is no multiple of 16; the records of the same film are 16 pieces and a tail."""
    import torch
    n = 1449
    assert n * n * 4 == (8 << 20) + 9796 and n * n * 64 > 16 * (8 << 20)
    with api.Renderer(scenes.cornell_box(n, n)) as r:
        r.render(0, 1)
        got = r.rgb8(alpha=True)
        t = r.rgb8_into(torch.full((n, n, 4), 0xAB, dtype=torch.uint8, device="cuda"), alpha=True)
        r.sync()
        assert got[..., :3].any() and got.tobytes() == t.cpu().numpy().tobytes()
        got = r.gbuffer(0, 1)
        t = r.gbuffer_into(torch.full((n * n * 64,), 0xAB, dtype=torch.uint8, device="cuda"), 0, 1)
        r.sync()
        assert (got["n"] == 1).all() and got.tobytes() == t.cpu().numpy().tobytes()


def test_a_shards_packed_buffer_downloads_as_it_lies_on_the_device():
    s = scenes.cornell_box(100, 70)
    for rank in range(3):
        with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            r.render(0, 12)
            r.denoise_shard_prepare()
            got = r.download_denoise_shard()
            ptr, n = r.denoise_shard_buffer()
            assert n == got.nbytes == api.denoise_shard_bytes(100, 70, rank, 3) and got.any()
            assert got.tobytes() == device_bytes(ptr, n).tobytes()

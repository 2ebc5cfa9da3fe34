"""GPU: the passes over the eight frame chains -- the resolve behind rene_download, rene_download_mean, rene_estimate_noise,
rene_resolve_robust, rene_export_features, the prepare pass of rene_denoise -- fed with CRAFTED chains through rene_load_chains instead of
what a render happened to leave: ties, NaN, infinities, overflow, denormals, -0.0 and negative sums, every rounding boundary of fp16, full
groups of sixteen workgroups, ragged tiles one pixel wide, uneven tiles with a zero tile, and tile sums held to the fixed reduction order bit
for bit.  tests/test_chain_reference.py asserts on the CPU that the films contain these classes; nothing here renders, apart from the one test
that ties the probe to a render.

"Bit for bit" (chain_reference.differing): where the restatement is a NaN the device must give a NaN -- payload and sign are free, x86 and the
device produce different default NaNs -- and everywhere else the bits are equal, so -0.0 differs from 0.0."""
import ctypes as C

import numpy as np
import pytest

import adaptive_reference as ar
import atrous_reference as atr
import chain_reference as cr
import features_reference as fr
import noise_reference as nr
import robust_reference as rr
import test_gpu_denoise
import test_gpu_noise
import test_gpu_robust
from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

H, W = 130, 161      # 5 x 6 = 30 tiles: one full group of 16 workgroups and a remainder of 14; the last column 1 pixel wide, the last row 2 high
SH, SW = 64, 512     # 32 tiles, for the sweeps
FIRST = 3
ALL = fr.ALL
MASKS = {"all": ALL, "default": fr.DEFAULT, "variance|frames": fr.VARIANCE | fr.FRAMES, "half_b": fr.HALF_B}


@pytest.fixture(scope="module")
def films():
    edge, finite, where = cr.edge_chains(H, W, seed=0)
    return {"edge": edge, "finite": finite, "where": where}


def edge_scene():
    return scenes.cornell_box(W, H)


def sweep_scene():
    return scenes.cornell_box(SW, SH)


def same(got, want, label):
    """Asserts bit-for-bit equality under the rule above; prints and returns the number of elements compared."""
    d = cr.differing(got, want)
    n = int(d.sum())
    print(f"{label}: {n} of {d.size} elements differ ({int(np.isnan(want).sum())} NaN, {int((np.signbit(want) & (want == 0)).sum())} -0.0 in the restatement)")
    assert n == 0, (label, n, np.argwhere(d)[:4].tolist())
    return d.size


def raw(t):
    """A record array's bits: [...][4] u32."""
    return np.ascontiguousarray(t).view(np.uint32).reshape(t.shape + (4,))


def uneven_frames():
    """Tile frame counts of four classes over the film's grid -- 0, 11, 19 and 35 frames, tests/adaptive_reference.py's schedule."""
    return ar.class_frames(ar.tile_classes(W, H))


def mean_of(sums, tile_frames):
    """rene_download_mean of [H][W][3] sums: every pixel divided by (float)N_t of its tile, IEEE; 0 where the tile has no frames."""
    out = np.zeros_like(sums)
    with np.errstate(all="ignore"):
        for (ty, tx), nt in np.ndenumerate(np.asarray(tile_frames)):
            sl = (slice(ty * 32, (ty + 1) * 32), slice(tx * 32, (tx + 1) * 32))
            if nt:
                out[sl] = sums[sl] / np.float32(nt)
    return out


# ---- a. the load is the identity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("film", ["finite", "edge"])
@pytest.mark.parametrize("schedule", ["uniform", "tiles"])
def test_load_is_the_identity(films, film, schedule):
    if schedule == "uniform":
        n, tf = 12, None
        chains = cr.for_counts(films[film], cr.chain_counts(n, FIRST))
        frames = np.full(cr.tile_grid(H, W), n, np.uint32)
    else:
        n, tf = 35, uneven_frames()
        assert (tf == 0).any() and (tf == n).any() and len(np.unique(tf)) == 4
        chains = cr.for_tile_frames(films[film], FIRST, tf)
        frames = tf
    want = cr.resolve(chains)
    with api.Renderer(edge_scene()) as r:
        r.load_chains(chains, FIRST, n, tf)
        assert np.array_equal(r.tile_frames(), frames)
        st = r.stats()
        assert st.frames == n and st.paths == 0 and st.launches == 0
        for l in range(3):
            same(r.download(l), want[l], f"{film}/{schedule}: download({l})")
            same(r.download_mean(l), mean_of(want[l], frames), f"{film}/{schedule}: download_mean({l})")
        d4 = r.download(0, channels=4)
        same(d4[..., :3], want[0], f"{film}/{schedule}: download(0, channels=4)")
        assert not d4[..., 3].any()
        met = {k: int(v.sum()) for k, v in films["where"].items()} if film == "edge" else "the finite classes"
        print(f"{film}/{schedule}: classes met (pixels) {met}")


def rendered_chains(r, spp):
    """The chains of every layer a job of frames 0 .. spp - 1 leaves on the device, rebuilt the way tests/test_gpu_noise.py rebuilds layer 0:
    chain c alone rendered into a reset context -- the other chains hold 0, adding 0 is exact, the download IS the chain."""
    chains = np.zeros((8, 3, r.yres, r.xres, 3), np.float32)
    for c in range(8):
        r.reset()
        for f in range(c, spp, 8):
            r.render(f, 1)
        for l in range(3):
            chains[c, l] = r.download(l)
    return chains


def test_loaded_chains_are_a_renders_chains():
    """The probe leaves the state a render leaves: Cornell 100 x 70, 12 frames, its chains rebuilt and loaded into a second context -- every
    hand-out of every pass is bit-identical to the rendering context's."""
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r, api.Renderer(s) as loaded:
        chains = rendered_chains(r, 12)
        r.reset()
        r.render(0, 12)
        loaded.load_chains(chains, 0, 12)
        assert loaded.stats().frames == r.stats().frames == 12 and np.array_equal(loaded.tile_frames(), r.tile_frames())
        n = 0
        for l in range(3):
            n += same(loaded.download(l), r.download(l), f"download({l})")
            n += same(loaded.download_mean(l), r.download_mean(l), f"download_mean({l})")
        assert loaded.estimate_noise().as_dict() == r.estimate_noise().as_dict()
        assert np.array_equal(raw(loaded.noise_tiles()), raw(r.noise_tiles()))
        sa, sb = loaded.resolve_robust(), r.resolve_robust()
        assert all(getattr(sa, k) == getattr(sb, k) for k, _ in abi.RobustSummary._fields_)
        n += same(loaded.download_robust(), r.download_robust(), "robust image")
        n += same(loaded.download_robust(abi.ROBUST_TRIM), r.download_robust(abi.ROBUST_TRIM), "robust j")
        assert np.array_equal(raw(loaded.robust_tiles()), raw(r.robust_tiles())) and (r.download_robust(abi.ROBUST_TRIM) > 0).any()
        for dtype, layout in (("f32", "hwc"), ("f16", "chw")):
            n += same(loaded.features(ALL, dtype, layout), r.features(ALL, dtype, layout), f"features {dtype} {layout}")
        loaded.denoise()
        r.denoise()
        n += same(loaded.download_denoised(), r.download_denoised(), "denoised")
        print(f"a load of a render's chains: {n} elements compared, 0 differ; noise, robust and feature records identical")


# ---- b. the robust resolve ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("film", ["edge", "finite"])
@pytest.mark.parametrize("spp", [12, 5, 16, 1])
def test_robust_resolve_on_crafted_chains(films, film, spp):
    """Image, j and the records' counts bit for bit at every max_trim and three gains; on the finite film the records' SUMS too, against the
    fixed reduction order of chain_pass.h restated (chain_reference.tile_reduce_order) -- no tolerance."""
    n_c = cr.chain_counts(spp, FIRST)
    chains = cr.for_counts(films[film], n_c)
    compared = 0
    hist = np.zeros(4, int)
    with api.Renderer(edge_scene()) as r:
        r.load_chains(chains, FIRST, spp)
        for max_trim in range(4):
            for gain in (0.5, 1.0, 3.0):
                label = f"{film}, {spp} frames, max_trim {max_trim}, gain {gain}"
                want = rr.resolve(chains[:, 0], n_c, max_trim=max_trim, gain=gain, dtype=np.float32)
                summ = r.resolve_robust(max_trim=max_trim, gain=gain)
                img, j, tiles = r.download_robust(), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles()
                d_img, d_j = cr.differing(img, want["image"]).any(axis=-1), cr.differing(j, want["j"].astype(np.float32))
                assert not d_img.any() and not d_j.any(), (label, int(d_img.sum()), int(d_j.sum()), np.argwhere(d_img | d_j)[:4].tolist())
                _, _, n, nt = rr.tile_records(want["lum_plain"], want["lum_robust"], want["j"])
                assert np.array_equal(tiles["n_pixels"], n) and np.array_equal(tiles["n_trimmed"], nt), label
                assert summ.n_pixels == H * W and summ.n_trimmed == int((want["j"] > 0).sum()) and summ.n_frames == spp
                if film == "finite":
                    for field, plane in (("sum_lum_plain", want["lum_plain"]), ("sum_lum_robust", want["lum_robust"])):
                        d = cr.differing(tiles[field], cr.tile_sums_in_order(plane))
                        assert not d.any(), (label, field, np.argwhere(d).tolist())
                compared += d_img.size
                hist += np.bincount(want["j"].ravel(), minlength=4)
    print(f"robust resolve, {film} film, {spp} frames from {FIRST}: 12 parameter sets, {compared} pixels compared, 0 differ in image or j; "
          f"j histogram over the sets {hist.tolist()}" + ("; tile sums equal the fixed-order restatement bit for bit" if film == "finite" else ""))


def test_robust_tile_shards_of_one_load(films):
    chains = cr.for_counts(films["edge"], cr.chain_counts(12, FIRST))
    s = edge_scene()
    owner = np.arange(30).reshape(5, 6) % 3
    owner_px = np.repeat(np.repeat(owner, 32, axis=0), 32, axis=1)[:H, :W]
    with api.Renderer(s) as whole:
        whole.load_chains(chains, FIRST, 12)
        whole.resolve_robust()
        img, j, tiles = whole.download_robust(), whole.download_robust(abi.ROBUST_TRIM), whole.robust_tiles()
        layers = [whole.download(l) for l in range(3)]
    for rank in range(3):
        with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=3) as r:
            r.load_chains(chains, FIRST, 12)
            summ = r.resolve_robust()
            mine = owner_px == rank
            si, sj, st = r.download_robust(), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles()
            same(si[mine], img[mine], f"shard {rank}: image of the owned tiles")
            same(sj[mine], j[mine], f"shard {rank}: j of the owned tiles")
            assert not si[~mine].view(np.uint32).any() and not sj[~mine].view(np.uint32).any()
            same(raw(st)[owner == rank].view(np.float32), raw(tiles)[owner == rank].view(np.float32), f"shard {rank}: records of the owned tiles")
            assert not raw(st)[owner != rank].any()
            assert summ.n_tiles == 10 and summ.n_pixels == int(mine.sum())
            for l in range(3):
                got = r.download(l)
                same(got[mine], layers[l][mine], f"shard {rank}: download({l}) of the owned tiles")
                assert not got[~mine].view(np.uint32).any()


# ---- c. the feature export ----------------------------------------------------------------------------------------------------------------------
def features_want(chains, first, tile_frames, mask, dtype, layout):
    """The restatement's tensor for loaded chains whose tiles hold tile_frames frames from `first`."""
    s = cr.resolve(chains)

    def make(nt):
        return fr.tensor(fr.features(chains[:, 0], cr.chain_counts(nt, first), s[1], s[2]), mask, "hwc")

    t = cr.per_tile(H, W, tile_frames, make)
    if dtype == "f16":
        t = fr.to_f16(t)
    return np.ascontiguousarray(t if layout == "hwc" else np.moveaxis(t, -1, 0))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_feature_export_on_the_edge_film(films, dtype, layout):
    """Every instantiation of the kernel on the edge film: 30 owned tiles, so the pairing permutation of the full group of sixteen workgroups
    and the plain order of the remaining fourteen both run; uniform tiles and uneven ones with a zero tile."""
    tf_uniform = np.full(cr.tile_grid(H, W), 12, np.uint32)
    tf_uneven = uneven_frames()
    loads = {"uniform": (cr.for_counts(films["edge"], cr.chain_counts(12, FIRST)), 12, None, tf_uniform),
             "uneven": (cr.for_tile_frames(films["edge"], FIRST, tf_uneven), 35, tf_uneven, tf_uneven)}
    n = 0
    with api.Renderer(edge_scene()) as r:
        for name, (chains, spp, tf, frames) in loads.items():
            r.reset()
            r.load_chains(chains, FIRST, spp, tf)
            for mname, mask in MASKS.items():
                want = features_want(chains, FIRST, frames, mask, dtype, layout)
                n += same(r.features(mask, dtype, layout), want, f"features {dtype} {layout} {mname}, {name} tiles")
    print(f"feature export {dtype} {layout}: {n} elements compared over 4 masks x (uniform, uneven) tiles, 0 differ")


def test_feature_export_writes_its_tensor_and_nothing_else(films):
    """A caller-owned buffer pre-filled with a sentinel, with slack behind the tensor: the C H W elements equal the restatement, no byte behind
    them changes -- from one context, and from three tile shards that fill the tensor between them."""
    import torch
    chains = cr.for_counts(films["edge"], cr.chain_counts(12, FIRST))
    frames = np.full(cr.tile_grid(H, W), 12, np.uint32)
    owner = np.repeat(np.repeat(np.arange(30).reshape(5, 6) % 3, 32, axis=0), 32, axis=1)[:H, :W]
    s = edge_scene()
    SENTINEL, SLACK = 0xA5, 4096
    ctxs = [api.Renderer(s)] + [api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=3) for k in range(3)]
    try:
        for r in ctxs:
            r.load_chains(chains, FIRST, 12)
        for dtype, npdt in (("f32", np.float32), ("f16", np.float16)):
            for layout in ("hwc", "chw"):
                want = features_want(chains, FIRST, frames, ALL, dtype, layout)
                p = api._feature_params(ALL, dtype, layout)
                label = f"{dtype} {layout}"

                def export(r, buf):
                    torch.cuda.synchronize()
                    api._check(api.lib().rene_export_features(r._h, C.byref(p), C.c_void_p(buf.data_ptr()), buf.numel()))
                    out = buf.cpu().numpy()
                    assert (out[want.nbytes:] == SENTINEL).all(), (label, "bytes behind the tensor were written")
                    return out[:want.nbytes].view(npdt).reshape(want.shape)

                buf = torch.full((want.nbytes + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda:0")
                same(export(ctxs[0], buf), want, f"caller-owned {label}, one context")
                buf = torch.full((want.nbytes + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda:0")
                sent = np.full(want.nbytes, SENTINEL, np.uint8).view(npdt).reshape(want.shape)
                px = (lambda a: a) if layout == "hwc" else (lambda a: np.moveaxis(a, 0, -1))
                for k in range(3):
                    got = export(ctxs[1 + k], buf)
                    done, todo = owner <= k, owner > k
                    same(px(got)[done], px(want)[done], f"caller-owned {label}, shards 0..{k}: their tiles")
                    assert np.array_equal(px(got)[todo].view(np.uint8), px(sent)[todo].view(np.uint8)), (label, k, "another shard's tiles were written")
    finally:
        for r in ctxs:
            r.close()


# ---- d. the fp16 converter, exhaustively --------------------------------------------------------------------------------------------------------
def test_fp16_converter_at_every_rounding_boundary():
    """Eight frames from 0: every chain holds one.  8 v in chain 0 and zeros of v's sign elsewhere make COLOR == v bit for bit (8 v and the
    division by 8 are exact); 4 v in chain 0 does the same for HALF_A.  All of half_ties() -- the midpoint of every pair of adjacent finite
    halves and its fp32 neighbours, both signs, the clamp's edge, infinities, NaN, the smallest halves, +-0 -- in both layouts."""
    v = cr.half_ties()
    parts = cr.value_films(v, SH, SW)
    n = ties = 0
    with api.Renderer(sweep_scene()) as r:
        for film in parts:
            want = fr.to_f16(film)
            ties += int(cr.is_half_tie(film).sum())
            for scale, mask, name in ((8, fr.COLOR, "COLOR"), (4, fr.HALF_A, "HALF_A")):
                r.reset()
                r.load_chains(cr.single_chain_load(film, scale), 0, 8)
                same(r.features(mask, "f32", "hwc"), film, f"{name} fp32 == v")
                for layout in ("hwc", "chw"):
                    n += same(r.features(mask, "f16", layout), want if layout == "hwc" else np.moveaxis(want, -1, 0), f"{name} f16 {layout} == to_f16(v)")
    print(f"fp16 converter: {v.size} fp32 values swept ({ties} exact ties, every pair of adjacent finite halves, both signs) through COLOR and HALF_A "
          f"in both layouts: {n} conversions compared, 0 differ")
    assert ties >= 60000


# ---- e. every slot counts once ------------------------------------------------------------------------------------------------------------------
def test_every_slot_counts_once():
    """512 x 64, 32 tiles, 32 loads: load i puts ONE hot pixel -- the same eight chain values every time -- at row-major position 32 i + t of
    tile t, zeros elsewhere.  Over the loads every one of the 1024 positions of a tile is visited; a sum of zeros and one value is that value
    in any order, so every tile's records must be bit-identical every time: a slot the reduction drops, or counts twice, shows."""
    n_c = cr.chain_counts(16, 0)
    hot = (np.array([1, 2, 3, 4, 5, 6, 7, 80], np.float32) * 2)[:, None] * np.array([1.0, 0.5, 0.25], np.float32)[None, :]  # [8][3]
    one = np.zeros((8, 32, 32, 3), np.float32)
    one[:, 0, 0] = hot
    w_noise = nr.estimate(one, n_c)
    w_rob = rr.resolve(one, n_c)
    a, b, _, nt = rr.tile_records(w_rob["lum_plain"], w_rob["lum_robust"], w_rob["j"])
    first_noise = first_rob = None
    visited = np.zeros((32, 1024), int)
    chains = np.zeros((8, 3, SH, SW, 3), np.float32)
    with api.Renderer(sweep_scene()) as r:
        for i in range(32):
            chains[:, 0] = 0
            for t in range(32):
                p = 32 * i + t
                y, x = (t // 16) * 32 + p // 32, (t % 16) * 32 + p % 32
                chains[:, 0, y, x] = hot
                visited[t, cr.slot_of(p % 32, p // 32)] += 1
            r.reset()
            r.load_chains(chains, 0, 16)
            est = r.estimate_noise()
            noise = r.noise_tiles()
            r.resolve_robust()
            rob = r.robust_tiles()
            if i == 0:
                first_noise, first_rob = raw(noise)[0, 0], raw(rob)[0, 0]
                for got, want in ((noise["sum_var"][0, 0], w_noise["A"][0, 0]), (noise["sum_lum"][0, 0], w_noise["B"][0, 0])):
                    assert abs(got - want) / (2 * abs(want)) <= test_gpu_noise.BOUND, (got, want)   # |value| + the largest tile's value: the same tile
                for got, want in ((rob["sum_lum_plain"][0, 0], a[0, 0]), (rob["sum_lum_robust"][0, 0], b[0, 0])):
                    assert abs(got - want) / (2 * abs(want)) <= test_gpu_robust.BOUND, (got, want)
                assert rob["n_trimmed"][0, 0] == nt[0, 0] == 1 and w_noise["A"][0, 0] > 0
            assert (raw(noise) == first_noise).all(), (i, np.argwhere((raw(noise) != first_noise).any(axis=-1)).tolist())
            assert (raw(rob) == first_rob).all(), (i, np.argwhere((raw(rob) != first_rob).any(axis=-1)).tolist())
            assert (noise["n_pixels"] == 1024).all() and (rob["n_pixels"] == 1024).all() and est.n_pixels == SH * SW
    assert (visited.sum(axis=0) == 1).all()  # all 1024 slots, each once over the tiles
    print(f"every slot once: 32 loads x 32 tiles, the hot pixel in each of the 1024 slots; noise record {first_noise.tolist()} and robust record "
          f"{first_rob.tolist()} (bits) identical in all 1024 cases")


# ---- f. the noise estimate and the denoiser -----------------------------------------------------------------------------------------------------
def noise_errors(tiles, want, pick):
    scale_a, scale_b = want["A"].max(), want["B"].max()
    a, b = tiles["sum_var"].astype(np.float64), tiles["sum_lum"].astype(np.float64)
    err_a = (np.abs(a - want["A"]) / (np.abs(want["A"]) + scale_a))[pick]
    err_b = (np.abs(b - want["B"]) / (np.abs(want["B"]) + scale_b))[pick]
    return float(err_a.max()), float(err_b.max())


def test_noise_estimate_and_denoiser_on_the_finite_film(films):
    """Held to tests/noise_reference.py and tests/atrous_reference.py with the bounds tests/test_gpu_noise.py and tests/test_gpu_denoise.py carry."""
    n_c = cr.chain_counts(12, FIRST)
    chains = cr.for_counts(films["finite"], n_c)
    s = cr.resolve(chains)
    with api.Renderer(edge_scene()) as r:
        r.load_chains(chains, FIRST, 12)
        est = r.estimate_noise()
        tiles = r.noise_tiles()
        want = nr.estimate(chains[:, 0], n_c, floor=est.luminance_floor)
        assert np.array_equal(tiles["n_pixels"], want["n"]) and est.n_frames == 12 and est.n_chains == 8 and est.n_pixels == H * W
        ea, eb = noise_errors(tiles, want, np.ones(want["n"].shape, bool))
        print(f"noise estimate on the finite film: sum_var max err {ea:.3g}, sum_lum max err {eb:.3g} of |value| + largest tile (bound {test_gpu_noise.BOUND:.3g})")
        assert ea <= test_gpu_noise.BOUND and eb <= test_gpu_noise.BOUND
        fig = nr.figures(tiles["sum_var"], tiles["sum_lum"], tiles["n_pixels"], est.luminance_floor)
        for k in ("sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse", "worst_tile_noise"):
            assert abs(getattr(est, k) - fig[k]) <= 1e-12 * abs(fig[k]), k
        assert est.worst_tile == fig["worst_tile"]
        r.denoise()
        got, got_var = r.download_denoised().astype(np.float64), r.download_denoised(abi.DENOISED_VARIANCE).astype(np.float64)
        w, w_var = atr.denoise(chains[:, 0], n_c.astype(np.float64), s[1], s[2])
        bound = test_gpu_denoise.BOUND
        err = np.abs(got / 12 - w / 12) / (1 + np.abs(w / 12))
        verr = np.abs(got_var - w_var) - bound * np.abs(w_var)
        print(f"denoiser on the finite film: radiance max err {err.max():.3g} of 1 + |value| (bound {bound:.3g}); variance max |diff| - rtol |v| = "
              f"{verr.max():.3g} against atol {bound * w_var.max():.3g}")
        assert np.isfinite(got).all() and err.max() <= bound and (verr <= bound * w_var.max()).all()
        for l in range(3):
            same(r.download(l), s[l], f"download({l}) after the passes")  # read, never written


def test_noise_estimate_on_uneven_loaded_tiles(films):
    """Uneven tiles: every tile is estimated with the constants of its own N_t -- its record is the restatement's for N_t frames within the
    bound, and bit for bit the record of a uniform load of N_t frames; tiles without frames are not estimated."""
    tf = uneven_frames()
    chains = cr.for_tile_frames(films["finite"], FIRST, tf)
    s = edge_scene()
    with api.Renderer(s) as r, api.Renderer(s) as u:
        r.load_chains(chains, FIRST, 35, tf)
        est = r.estimate_noise()
        tiles = r.noise_tiles()
        assert est.n_frames == 35 and est.n_tiles == int((tf > 0).sum())
        assert not raw(tiles)[tf == 0].any()
        for nt in (11, 19, 35):
            n_c = cr.chain_counts(nt, FIRST)
            uniform = cr.for_counts(films["finite"], n_c)
            want = nr.estimate(uniform[:, 0], n_c, floor=est.luminance_floor)
            pick = tf == nt
            assert np.array_equal(tiles["n_pixels"][pick], want["n"][pick])
            ea, eb = noise_errors(tiles, want, pick)
            print(f"uneven tiles, N_t = {nt} ({int(pick.sum())} tiles): sum_var max err {ea:.3g}, sum_lum max err {eb:.3g} (bound {test_gpu_noise.BOUND:.3g})")
            assert ea <= test_gpu_noise.BOUND and eb <= test_gpu_noise.BOUND
            u.reset()
            u.load_chains(uniform, FIRST, nt)
            u.estimate_noise()
            assert np.array_equal(raw(tiles)[pick], raw(u.noise_tiles())[pick]), nt
        fig = nr.figures(tiles["sum_var"], tiles["sum_lum"], tiles["n_pixels"], est.luminance_floor)
        for k in ("sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse", "worst_tile_noise"):
            assert abs(getattr(est, k) - fig[k]) <= 1e-12 * abs(fig[k]), k
        with pytest.raises(api.ReneError) as e:
            r.denoise()
        assert e.value.code == -4  # its steps take one N


def test_noise_estimate_and_denoiser_take_the_edge_film(films):
    """Their specifications say nothing about non-finite input: they return, and leave the accumulation state as it is."""
    chains = cr.for_counts(films["edge"], cr.chain_counts(12, FIRST))
    s = cr.resolve(chains)
    with api.Renderer(edge_scene()) as r:
        r.load_chains(chains, FIRST, 12)
        est = r.estimate_noise()
        assert est.n_pixels == H * W and (r.noise_tiles()["n_pixels"] > 0).all()
        r.denoise()
        assert r.download_denoised().shape == (H, W, 3)
        for l in range(3):
            same(r.download(l), s[l], f"download({l}) after the noise estimate and the denoiser")


# ---- g. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    s = scenes.cornell_box(100, 70)
    L = api.lib()
    n_floats = 8 * 3 * 70 * 100 * 3
    rng = np.random.default_rng(5)
    chains = rng.uniform(0, 2, (8, 3, 70, 100, 3)).astype(np.float32)
    ptr = chains.ctypes.data_as(C.c_void_p)

    def call(r, p=ptr, n=n_floats, first=0, frames=8, tf=None, n_tiles=0):
        rc = L.rene_load_chains(r._h if r is not None else None, p, n, first, frames, None if tf is None else tf.ctypes.data_as(C.c_void_p), n_tiles)
        assert rc == 0 or L.rene_last_error()  # a message
        return rc

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        return e.value.code

    tf = np.full(12, 8, np.uint32)
    with api.Renderer(s) as r, api.Renderer(s) as fresh:
        assert call(None) == -1 and call(r, p=None) == -1              # a NULL argument
        assert call(r, n=n_floats - 1) == -1                           # n_floats too small
        assert call(r, frames=0) == -1                                 # no frames
        assert call(r, first=0xffffffff, frames=2) == -1               # the frame range leaves u32
        assert call(r, tf=tf, n_tiles=11) == -1                        # not the grid
        bad = tf.copy()
        bad[5] = 9
        assert call(r, tf=bad, n_tiles=12) == -1                       # a tile with more than n_frames
        assert call(r, tf=np.full(12, 7, np.uint32), n_tiles=12) == -1  # no tile with n_frames
        with pytest.raises(ValueError):
            r.load_chains(chains[:, :, :69])                           # the Python side's own check
        with pytest.raises(ValueError):
            r.load_chains(chains, tile_frames=np.zeros((4, 3)))
        # nothing was written: the context is as fresh as it was
        assert r.stats().frames == 0 and not r.tile_frames().any() and not r.download(0).view(np.uint32).any()
        r.render(0, 4)
        before = r.download(0)
        assert call(r) == -1 and b"already holds frames" in L.rene_last_error()
        assert np.array_equal(r.download(0), before) and r.stats().frames == 4
        r.reset()
        assert call(r) == 0                                            # a reset context takes a load
        same(r.download(0), cr.resolve(chains)[0], "download(0) after the refusals")
        assert call(r) == -1 and b"already holds frames" in L.rene_last_error()   # ... one
        assert code(lambda: r.render(8, 1)) == -4 and code(lambda: r.render(0, 0)) == -4   # nothing renders onto loaded chains
        assert code(lambda: r.set_active_tiles(np.ones((3, 4)))) == -4
        same(r.download(0), cr.resolve(chains)[0], "download(0) after the refused render")
        assert r.estimate_noise().n_frames == 8                        # the reading calls go on working
        r.reset()
        r.render(0, 4)                                                 # until the reset
        fresh.render(0, 4)
        assert np.array_equal(r.download(0), fresh.download(0)) and np.array_equal(r.download(0), before)
        r.set_active_tiles(np.ones((3, 4)))
        # an exchange consumes the chains
        r.reset()
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 8)
        r.gather_tiles(0)
        assert call(r) == -4
        r.reset()
        assert call(r, tf=tf, n_tiles=12) == 0 and r.stats().frames == 8
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        assert call(r) == -4                                           # a frame shard holds a share of every pixel's frames
        r.render(0, 4)
        assert r.download(0).max() > 0
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=1) as r:  # shard_count 1 is unsharded, whatever the mode
        assert call(r) == 0 and r.stats().frames == 8

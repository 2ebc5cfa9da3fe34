"""Test helper (not a conftest): the per-pixel records of the light-group pass (rene_lights, include/rene_hip.h) and the figures api.py makes of
them, restated in numpy operation by operation, and the CPU oracle's renders of a scene with all but one group of sources black.

`pixel_records` turns the per-sample records of rene_lights_samples into pixel records by the header's words: per pixel, in frame order,
group[g].sum + sample.group[g].sum -- a plain fp32 add per component, of every sample (one that has nothing for a group holds + 0 there) -- the
integer sums adds and lit, and n, the samples of the pixel (0 where the context does not own it: its samples are the all-zero record).
`total`, `group_mean`, `mix` and `merge` restate api.lights_sum, lights_group_mean, lights_mix and lights_merge.  `crafted` makes one pixel's
sample list by hand.

`oracle_only(name, builder, g, n_frames, oracle_mod)` renders the builder's scene with every source outside group g black (g None: the full
scene) on the CPU oracle, once per process: the image's sums, the same radiance summed in doubles, and the counters."""
import numpy as np

import lights_scenes
from rene_amd import abi

GROUPS = abi.LIGHTS_GROUPS


def pixel_records(samples) -> np.ndarray:
    """samples: (n_frames, H, W) records of abi.LIGHTS_SAMPLE_DTYPE -> (H, W) records of abi.LIGHTS_DTYPE."""
    samples = np.asarray(samples)
    assert samples.dtype == np.dtype(abi.LIGHTS_SAMPLE_DTYPE) and samples.ndim == 3
    n, H, W = samples.shape
    out = np.zeros((H, W), abi.LIGHTS_DTYPE)
    sums = np.zeros((H, W, GROUPS, 3), np.float32)
    for f in range(n):
        sums = sums + samples["group"]["sum"][f].astype(np.float32)  # fp32 + fp32 -> fp32, rounded once
        out["group"]["adds"] += samples["group"]["adds"][f]
        out["n"] += samples["n"][f]
        out["lit"] += samples["lit"][f]
    out["group"]["sum"] = sums
    return out


def total(rec) -> np.ndarray:
    """((g0 + g1) + g2) + ... over the eight groups, every add rounded to fp32."""
    sums = np.asarray(rec)["group"]["sum"]
    out = sums[..., 0, :].astype(np.float32)
    for g in range(1, GROUPS):
        out = (out + sums[..., g, :]).astype(np.float32)
    return out


def _per_sample(rec, value) -> np.ndarray:
    out = np.zeros(value.shape, np.float32)
    n = np.asarray(rec)["n"]
    own = n != 0
    with np.errstate(invalid="ignore", over="ignore"):
        out[own] = (value[own] / n[own].astype(np.float32)[:, None]).astype(np.float32)
    return out


def group_mean(rec, g) -> np.ndarray:
    return _per_sample(rec, np.asarray(rec)["group"]["sum"][..., g, :].astype(np.float32))


def mix(rec, weights) -> np.ndarray:
    """(((w0 g0) + (w1 g1)) + ... + (w7 g7)) / n, every product, add and the division one fp32 operation; 0 where n == 0."""
    w = np.asarray(weights, np.float32)
    w = np.broadcast_to(w.reshape(GROUPS, -1), (GROUPS, 3))
    sums = np.asarray(rec)["group"]["sum"]
    with np.errstate(invalid="ignore", over="ignore"):
        out = (w[0] * sums[..., 0, :]).astype(np.float32)
        for g in range(1, GROUPS):
            out = (out + (w[g] * sums[..., g, :]).astype(np.float32)).astype(np.float32)
    return _per_sample(rec, out)


def merge(parts) -> np.ndarray:
    out = np.zeros(parts[0].shape, parts[0].dtype)
    for p in parts:
        own = p["n"] != 0
        assert not out["n"][own].any()
        out[own] = p[own]
    return out


def crafted(values, adds=None, lit=None, length=None, end=None) -> np.ndarray:
    """A (n_frames, 1, 1) sample array for one pixel: values[f][g] is the sample's value for group g ((n_frames, 8, 3), or (n_frames, 8) for the
    red channel alone), adds[f][g] the counts (default 1 where the value is not 0), lit[f] (default: any add), length[f] (default 1), end[f]
    (default MISS)."""
    values = np.asarray(values, np.float32)
    if values.ndim == 2:
        values = np.stack([values, np.zeros_like(values), np.zeros_like(values)], axis=-1)
    s = np.zeros((len(values), 1, 1), abi.LIGHTS_SAMPLE_DTYPE)
    s["group"]["sum"][:, 0, 0] = values
    s["group"]["adds"][:, 0, 0] = (values != 0).any(axis=-1) if adds is None else np.asarray(adds, np.uint32)
    s["n"] = 1
    s["lit"][:, 0, 0] = (s["group"]["adds"][:, 0, 0].sum(axis=-1) != 0) if lit is None else np.asarray(lit, np.uint32)
    s["length"][:, 0, 0] = 1 if length is None else np.asarray(length, np.uint32)
    s["end"][:, 0, 0] = abi.BOUNCES_END_MISS if end is None else np.asarray(end, np.uint32)
    return s


_oracle = {}


def oracle_only(name, builder, g, n_frames, oracle_mod):
    """The CPU oracle's render over frames 0 .. n_frames - 1 of the builder's scene with every source outside group g black; g None: the scene as
    it is.  {"image": (H, W, 3) fp32, the image's sums as the oracle keeps them; "stats": its counters; "doubles": (H, W, 3) fp64, the same
    radiance summed in doubles}.  The oracle keeps its decomposition in doubles but hands every layer out rounded to fp32, so "doubles" is read
    out ONE FRAME AT A TIME -- a frame's (depth, branch) layer of a pixel holds the one or two adds of one iteration, which the hand-out
    leaves exact or all but exact -- and added up here in fp64.  Once per process."""
    if (name, g) not in _oracle:
        scene = builder() if g is None else lights_scenes.only(builder, g)
        o = oracle_mod.Oracle(scene)
        o.set_experiment(decomposition=True)
        doubles = np.zeros((scene.film.yresolution, scene.film.xresolution, 3), np.float64)
        for f in range(n_frames):
            o.reset()
            o.render(f, 1)
            for d in range(10):
                for b in range(2):
                    doubles += o.download_decomposition(d, b)
        o.reset()
        o.render(0, n_frames)
        _oracle[name, g] = {"image": o.download(0)[..., :3].copy(), "doubles": doubles, "stats": o.stats().as_dict()}
        o.close()
    return _oracle[name, g]

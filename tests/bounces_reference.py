"""Test helper (not a conftest): the per-pixel records of the bounce pass (rene_bounces, include/rene_hip.h) restated in numpy, and the CPU oracle's
decomposition by bounce in the form the pass's tests hold it against.

`pixel_records` turns the per-sample records of rene_bounces_samples into pixel records by the header's last paragraph: per pixel, in frame order,
bucket[d].sum + sample.bucket[d].sum -- a plain fp32 add per component, of every sample (one that has nothing for a bucket holds + 0 there) --
the integer sums reached, length_sum and capped, the maximum length_max, and n, the samples of the pixel (0 where the context does not own it:
its samples are the all-zero record).  `sum_upto` restates api.bounces_sum.  `crafted` makes one pixel's sample list by hand.

`decomposition` runs the oracle once per scene with Oracle.set_experiment(decomposition=True) and keeps, per scene and process, the ten depth
layers (both branches added, fp64 as the oracle keeps them), the uncapped image and the counters; `cumulative` adds the first k layers."""
import numpy as np

from rene_amd import abi

BUCKETS = abi.BOUNCES_BUCKETS
MISS, PDF, ZERO, ROULETTE, CAP = abi.BOUNCES_END_MISS, abi.BOUNCES_END_PDF, abi.BOUNCES_END_ZERO, abi.BOUNCES_END_ROULETTE, abi.BOUNCES_END_CAP


def pixel_records(samples) -> np.ndarray:
    """samples: (n_frames, H, W) records of abi.BOUNCES_SAMPLE_DTYPE -> (H, W) records of abi.BOUNCES_DTYPE."""
    samples = np.asarray(samples)
    assert samples.dtype == np.dtype(abi.BOUNCES_SAMPLE_DTYPE) and samples.ndim == 3
    n, H, W = samples.shape
    out = np.zeros((H, W), abi.BOUNCES_DTYPE)
    sums = np.zeros((H, W, BUCKETS, 3), np.float32)
    for f in range(n):
        sums = sums + samples["bucket"]["sum"][f].astype(np.float32)  # fp32 + fp32 -> fp32, rounded once
        out["bucket"]["reached"] += samples["bucket"]["reached"][f]
        out["n"] += samples["n"][f]
        out["length_sum"] += samples["length"][f]
        out["length_max"] = np.maximum(out["length_max"], samples["length"][f])
        out["capped"] += ((samples["end"][f] == CAP) & (samples["n"][f] != 0)).astype(np.uint32)
    out["bucket"]["sum"] = sums
    return out


def sum_upto(rec, upto=BUCKETS) -> np.ndarray:
    """((b0 + b1) + b2) + ... over the first `upto` buckets, every add rounded to fp32."""
    sums = np.asarray(rec)["bucket"]["sum"]
    out = np.zeros(sums.shape[:-2] + (3,), np.float32)
    for d in range(upto):
        out = (out + sums[..., d, :]).astype(np.float32) if d else sums[..., 0, :].astype(np.float32)
    return out


def crafted(values, reached=None, length=None, end=None) -> np.ndarray:
    """A (n_frames, 1, 1) sample array for one pixel: values[f][d] is v[d] of frame f ((n_frames, 10, 3), or (n_frames, 10) for the red channel
    alone), reached[f][d] the counts (default 1 where v[d] != 0), length[f] (default the counts' sum), end[f] (default MISS)."""
    values = np.asarray(values, np.float32)
    if values.ndim == 2:
        values = np.stack([values, np.zeros_like(values), np.zeros_like(values)], axis=-1)
    s = np.zeros((len(values), 1, 1), abi.BOUNCES_SAMPLE_DTYPE)
    s["bucket"]["sum"][:, 0, 0] = values
    s["bucket"]["reached"][:, 0, 0] = (values != 0).any(axis=-1) if reached is None else np.asarray(reached, np.uint32)
    s["n"] = 1
    s["length"][:, 0, 0] = s["bucket"]["reached"][:, 0, 0].sum(axis=-1) if length is None else np.asarray(length, np.uint32)
    s["end"][:, 0, 0] = MISS if end is None else np.asarray(end, np.uint32)
    return s


_decomposition = {}


def decomposition(name, scene, n_frames, oracle_mod):
    """{"layers": (10, H, W, 3) fp64, "image": (H, W, 3) fp32 sums of the uncapped render, "stats": the oracle's counters}; once per process."""
    if name not in _decomposition:
        o = oracle_mod.Oracle(scene)
        o.set_experiment(decomposition=True)
        o.render(0, n_frames)
        layers = np.stack([o.download_decomposition(d, 0).astype(np.float64) + o.download_decomposition(d, 1).astype(np.float64) for d in range(BUCKETS)])
        _decomposition[name] = {"layers": layers, "image": o.download(0)[..., :3].copy(), "stats": o.stats().as_dict()}
    return _decomposition[name]


def cumulative(dec, k) -> np.ndarray:
    """The oracle's adds at iterations 0 .. k - 1 (k = 10: all of them), (H, W, 3) fp32."""
    return dec["layers"][:k].sum(axis=0).astype(np.float32)

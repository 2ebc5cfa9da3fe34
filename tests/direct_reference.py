"""Test helper (not a conftest): the per-pixel sums of the direct-light pass (rene_direct, include/rene_hip.h) restated in numpy.

`aggregate` turns the per-sample records of rene_direct_samples into pixel records by the header's last paragraph: per pixel, in frame order,
seen + sample.seen, distant + sample.distant and sampled + sample.sampled -- a plain fp32 add per component, of every sample (one that has nothing
for a sum holds + 0 there) -- and hits + 1 per sample whose state is not MISS.  `crafted` makes one pixel's sample list by hand."""
import numpy as np

from rene_amd import abi

MISS, LIGHT, BSDF, PLAIN, ENDED_PDF, ENDED_ZERO = (abi.DIRECT_MISS, abi.DIRECT_LIGHT, abi.DIRECT_BSDF, abi.DIRECT_PLAIN, abi.DIRECT_ENDED_PDF,
                                                   abi.DIRECT_ENDED_ZERO)


def aggregate(samples, owned=None) -> np.ndarray:
    """samples: (n_frames, H, W) records of abi.DIRECT_SAMPLE_DTYPE.  owned: (H, W) bool, the pixels of the tiles the context owns (default all);
    the others get the all-zero record."""
    samples = np.asarray(samples)
    n, H, W = samples.shape
    out = np.zeros((H, W), abi.DIRECT_DTYPE)
    hits = np.zeros((H, W), np.uint32)
    sums = {k: np.zeros((H, W, 3), np.float32) for k in ("seen", "distant", "sampled")}
    for f in range(n):
        hits += samples["state"][f] != MISS
        for k in sums:
            sums[k] = sums[k] + samples[k][f].astype(np.float32)  # fp32 + fp32 -> fp32, rounded once
    out["hits"], out["n"] = hits, n
    for k in sums:
        out[k] = sums[k]
    if owned is not None:
        out[~np.asarray(owned, bool)] = np.zeros((), abi.DIRECT_DTYPE)
    return out


def crafted(states, seen=None, distant=None, sampled=None) -> np.ndarray:
    """A (n_frames, 1, 1) sample array for one pixel: states[f] and the three contributions of every frame, (n_frames, 3) each (default 0)."""
    states = np.asarray(states, np.uint32)
    s = np.zeros((len(states), 1, 1), abi.DIRECT_SAMPLE_DTYPE)
    s["state"][:, 0, 0] = states
    for k, v in (("seen", seen), ("distant", distant), ("sampled", sampled)):
        if v is not None:
            s[k][:, 0, 0] = np.asarray(v, np.float32)
    return s

"""Test helper (not a conftest): the occlusion pass (rene_occlusion, include/rene_hip.h) restated in numpy.

`aggregate` turns the per-ray records of rene_occlusion_samples into pixel records by step 4 of the header: per pixel, in frame order and within a
frame in ray order, hits + 1 per hitting sample, rays + 1 and occluded + verdict per ray cast, and bent_sum + w -- a plain fp32 add per component --
for the unoccluded rays only.  `direction` is the occlusion ray's direction in fp64: random_cosine_direction (math.rs:45-56) of the two draws,
carried into the frame of n by bsdf_reference.onb_from_w (onb.rs:14-26)."""
import numpy as np

import bsdf_reference as br
from rene_amd import abi

MISS, OPEN, OCCLUDED, NO_RAY = abi.OCCLUSION_MISS, abi.OCCLUSION_OPEN, abi.OCCLUSION_OCCLUDED, abi.OCCLUSION_NO_RAY


def aggregate(samples, owned=None) -> np.ndarray:
    """samples: (n_frames, rays, H, W) records of abi.OCCLUSION_SAMPLE_DTYPE.  owned: (H, W) bool, the pixels of the tiles the context owns
    (default all); the others get the all-zero record."""
    samples = np.asarray(samples)
    n, rays, H, W = samples.shape
    out = np.zeros((H, W), abi.OCCLUSION_DTYPE)
    hits = np.zeros((H, W), np.uint32)
    cast = np.zeros((H, W), np.uint32)
    occluded = np.zeros((H, W), np.uint32)
    bent = np.zeros((H, W, 3), np.float32)
    for f in range(n):
        hits += samples["state"][f, 0] != MISS  # (a sample's rays share its first hit: the state is a miss for all of them or for none)
        for k in range(rays):
            state = samples["state"][f, k]
            w = samples["w"][f, k].astype(np.float32)
            cast += (state == OPEN) | (state == OCCLUDED)
            occluded += state == OCCLUDED
            bent = np.where((state == OPEN)[:, :, None], bent + w, bent)
    out["hits"], out["rays"], out["occluded"], out["n"], out["bent_sum"] = hits, cast, occluded, n, bent
    if owned is not None:
        out[~np.asarray(owned, bool)] = np.zeros((), abi.OCCLUSION_DTYPE)
    return out


def direction(n, r1, r2) -> np.ndarray:
    """(..., 3) fp64: to_world(onb_from_w(n), random_cosine_direction(r1, r2)) -- phi = 2 pi r1, (cos phi sqrt(r2), sin phi sqrt(r2), sqrt(1 - r2))
    on the frame's (u, v, w = n)."""
    n = np.asarray(n, np.float64)
    shape = n.shape[:-1]
    n = n.reshape(-1, 3)
    r1, r2 = np.asarray(r1, np.float64).reshape(-1), np.asarray(r2, np.float64).reshape(-1)
    s = np.sqrt(r2)
    x, y, z = np.cos(2.0 * np.pi * r1) * s, np.sin(2.0 * np.pi * r1) * s, np.sqrt(1.0 - r2)
    u, v, w = br.onb_from_w(n)
    return (x[:, None] * u + y[:, None] * v + z[:, None] * w).reshape(shape + (3,))


def crafted(states, ws=None) -> np.ndarray:
    """A (n_frames, rays, 1, 1) sample array for one pixel: states[f][k], and the directions ws[f][k] (default +z)."""
    states = np.asarray(states, np.uint32)
    s = np.zeros(states.shape + (1, 1), abi.OCCLUSION_SAMPLE_DTYPE)
    s["state"][:, :, 0, 0] = states
    s["w"][:, :, 0, 0] = (0.0, 0.0, 1.0) if ws is None else np.asarray(ws, np.float32)
    s["w"][s["state"] == MISS] = 0
    return s

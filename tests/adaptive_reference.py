"""Restatement of the adaptive job's host side (include/rene_hip.h: rene_noise_select_tiles) in plain numpy, and the mask schedule the GPU tests
of adaptive sampling share.  A helper for tests (like noise_reference.py): it does not import the library."""
import numpy as np

TILE = 32


def tile_q(sum_var, sum_lum, n_pixels, floor):
    """q_t = (A_t / n_t) / (B_t / n_t + floor)^2 in fp64, 0 where a tile has no pixels; the floor is held as fp32, as the library holds it."""
    a, b, n = np.asarray(sum_var, np.float64), np.asarray(sum_lum, np.float64), np.asarray(n_pixels, np.float64)
    q = np.zeros(a.shape, np.float64)
    ok = n > 0
    q[ok] = (a[ok] / n[ok]) / (b[ok] / n[ok] + float(np.float32(floor))) ** 2
    return q


def select_tiles(sum_var, sum_lum, n_pixels, active_in, floor, target, dilate):
    """The definition: a tile goes on if it is active-in, has pixels, and some tile within `dilate` steps of it (Chebyshev distance, itself
    included) is active-in, has pixels and sqrt(q) > target.  [ty][tx] uint8."""
    n = np.asarray(n_pixels)
    ty, tx = n.shape
    alive = (n > 0) if active_in is None else ((np.asarray(active_in) != 0) & (n > 0))
    noisy = alive & (np.sqrt(tile_q(sum_var, sum_lum, n_pixels, floor)) > target)
    out = np.zeros((ty, tx), np.uint8)
    for y in range(ty):
        for x in range(tx):
            near = noisy[max(0, y - dilate):y + dilate + 1, max(0, x - dilate):x + dilate + 1]
            out[y, x] = 1 if alive[y, x] and near.any() else 0
    return out


# ---- the schedule of the GPU tests: four classes of tiles with different frame counts ---------------------------------------------------------
# class A is switched off before the first render, B after a launch of 11 frames, C after one of 8 more, D renders the last 16 too: chains of
# unequal length (11 = 8 + 3, 19 = 16 + 3, 35 = 32 + 3) and launches that start in every phase of the chain rule
CLASS_FRAMES = {"A": 0, "B": 11, "C": 19, "D": 35}
LAUNCHES = (11, 8, 16)


def tile_grid(xres, yres):
    return (yres + TILE - 1) // TILE, (xres + TILE - 1) // TILE


def tile_classes(xres, yres):
    """[ty][tx] of 'A' .. 'D': class (x + y) mod 4 -- every class in the bottom row of a grid four tiles wide (the ragged row of an image whose
    height is no multiple of 32), all four present from a 3 x 2 grid on."""
    ty, tx = tile_grid(xres, yres)
    return np.array([["ABCD"[(x + y) % 4] for x in range(tx)] for y in range(ty)])


def class_frames(classes):
    return np.vectorize(CLASS_FRAMES.get)(classes).astype(np.uint32)


def tile_slices(xres, yres):
    """((ty, tx), (rows, columns)) of every tile, clipped to the image."""
    ty, tx = tile_grid(xres, yres)
    for y in range(ty):
        for x in range(tx):
            yield (y, x), (slice(y * TILE, min(yres, (y + 1) * TILE)), slice(x * TILE, min(xres, (x + 1) * TILE)))


def tile_pixels(xres, yres):
    n = np.zeros(tile_grid(xres, yres), np.int64)
    for t, (rows, cols) in tile_slices(xres, yres):
        n[t] = (rows.stop - rows.start) * (cols.stop - cols.start)
    return n


def run_schedule(r, classes):
    """The masked job on renderer r: A off, 11 frames, B off, 8 frames, C off, 16 frames."""
    mask = classes != "A"
    r.set_active_tiles(mask)
    done = 0
    for n, drop in zip(LAUNCHES, ("B", "C", None)):
        r.render(done, n)
        done += n
        if drop:
            mask = mask & (classes != drop)
            r.set_active_tiles(mask)

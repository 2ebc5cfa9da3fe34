#!/usr/bin/env python3
"""What firefly rejection inside the `atrous` denoiser buys, and at which gain: DESIGN.md section 4c's table for rene_denoise_robust.

For every scene, frame count and master seed (DEFAULT_SEED + 977 i, i = 0 .. 3): relMSE (tests/atrous_reference.py) of the plain mean, of the
plain filter and of the filter with the trimmed prepare at gains 0.25 / 0.35 / 0.5 / 0.7 / 1 -- the numpy restatements tests/atrous_reference.py
and tests/atrous_robust_reference.py in fp64 on the CPU oracle's chains -- against 1024 oracle frames from frame 100000 (default seed); the energy
kept (image mean over the reference's mean) and the share of pixels with j > 0.  No GPU is used.

    python tools/denoise_robust_study.py [--threads 8]
    python tools/denoise_robust_study.py --spread     the restatement's own fp32-vs-fp64 spread on the cases of tests/test_gpu_denoise_robust.py
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import atrous_reference as ar  # noqa: E402
import atrous_robust_reference as arr  # noqa: E402
import atrous_tiles_reference as at  # noqa: E402
from oracle import oracle  # noqa: E402
from rene_amd import abi, scenes  # noqa: E402

CASES = [("veach_mis(96, 54)", lambda: scenes.veach_mis(96, 54), (16, 64)),
         ("cornell_box(64, 64)", lambda: scenes.cornell_box(64, 64), (16, 64)),
         ("cornell_fog(64, 64)", lambda: scenes.cornell_fog(64, 64), (16, 64))]
SEEDS = [abi.DEFAULT_SEED + 977 * i for i in range(4)]
GAINS = (0.25, 0.35, 0.5, 0.7, 1.0)

# the uniform cases of tests/test_gpu_denoise_robust.py (scene, frames) and its uneven schedule, at both gains
SPREAD_UNIFORM = [("cornell_box(100, 70) @ 12", lambda: scenes.cornell_box(100, 70), 12), ("cornell_box(100, 70) @ 5", lambda: scenes.cornell_box(100, 70), 5),
                  ("veach_mis(96, 54) @ 32", lambda: scenes.veach_mis(96, 54), 32)]
SPREAD_GAINS = (1.0, 0.35)


def one_spread(label, chains, n_c, s1, s2, frames):
    for gain in SPREAD_GAINS:
        r32 = arr.denoise_robust(chains, n_c, s1, s2, gain=gain, dtype=np.float32)
        r64 = arr.denoise_robust(chains, n_c, s1, s2, gain=gain, decisions=(r32["j"], r32["kept"]))
        own = arr.denoise_robust(chains, n_c, s1, s2, gain=gain)
        s = float((np.abs(r32["mean"].astype(np.float64) - r64["mean"]) / (1 + np.abs(r64["mean"]))).max())
        print(f"{label}, gain {gain}: fp32 vs fp64 (the fp32 run's decisions) {s:.3g} of 1 + |mean|; 16 x = {16 * s:.3g}; pixels whose j differs between "
              f"the fp32 and the fp64 run's own decisions: {int((own['j'] != r32['j']).sum())} of {own['j'].size}; j > 0 on {float((r32['j'] > 0).mean()):.3f}", flush=True)


def spread(threads):
    for name, make, spp in SPREAD_UNIFORM:
        o = oracle.Oracle(make())
        chains, n_c, s1, s2 = ar.chains_of(o, spp, threads=threads)
        one_spread(name, chains, n_c, s1, s2, spp)
    o = oracle.Oracle(scenes.cornell_box(161, 130))
    classes = at.tile_classes(161, 130)
    parts = at.chains_by_count(o, set(at.CLASS_FRAMES.values()), threads=threads)
    film = at.compose({cl: parts[n] for cl, n in at.CLASS_FRAMES.items()}, classes, 130, 161)
    one_spread("cornell_box(161, 130), the five-class schedule", *film, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--spread", action="store_true")
    a = ap.parse_args()
    if a.spread:
        return spread(a.threads)
    heads = " | ".join(f"gain {g:g}" for g in GAINS)
    print(f"| scene @ frames | plain mean | plain filter | {heads} | pixels with j > 0 at 0.35 |")
    print("|---|---|---|" + "---|" * (len(GAINS) + 1))
    totals = np.zeros(len(GAINS))
    for name, make, marks in CASES:
        o = oracle.Oracle(make())
        o.render(100000, 1024, threads=a.threads)
        ref = o.download(0).astype(np.float64) / 1024
        rows = {m: [] for m in marks}
        for seed in SEEDS:
            chains = np.zeros((8, o.yres, o.xres, 3), np.float32)
            s1, s2 = np.zeros((o.yres, o.xres, 3), np.float32), np.zeros((o.yres, o.xres, 3), np.float32)
            for fr in range(max(marks)):
                o.reset()
                o.render(fr, 1, seed=seed, threads=a.threads)
                chains[fr % 8] += o.download(0)
                s1 += o.download(1)
                s2 += o.download(2)
                n = fr + 1
                if n not in marks:
                    continue
                n_c = at.chain_counts(0, n)
                plain = chains.astype(np.float64).sum(0) / n
                filt = ar.denoise(chains, n_c, s1, s2)[0] / n
                row = [ar.relmse(plain, ref), ar.relmse(filt, ref), float(filt.mean() / ref.mean())]
                for g in GAINS:
                    out = arr.denoise_robust(chains, n_c, s1, s2, gain=g)
                    row += [ar.relmse(out["mean"], ref), float(out["mean"].mean() / ref.mean())]
                    if g == 0.35:
                        share = float((out["j"] > 0).mean())
                rows[n].append(row + [share])
        for m in marks:
            r = np.array(rows[m])
            rng = lambda c: f"{r[:, c].min():.3g} – {r[:, c].max():.3g}"
            cells = [rng(0), f"{rng(1)} ({r[:, 2].mean():.2f})"] + [f"{rng(3 + 2 * i)} ({r[:, 4 + 2 * i].mean():.2f})" for i in range(len(GAINS))]
            print(f"| `{name}` @ {m} | " + " | ".join(cells) + f" | {r[:, -1].min():.2f} – {r[:, -1].max():.2f} |", flush=True)
            # which gain is best: the geometric mean over rows and seeds of relMSE(gain) / relMSE(plain filter)
            totals += np.array([np.log(r[:, 3 + 2 * i] / r[:, 1]).sum() for i in range(len(GAINS))])
    n_rows = sum(len(marks) for _, _, marks in CASES) * len(SEEDS)
    print("\ngeometric mean over all rows and seeds of relMSE(trimmed prepare) / relMSE(plain filter): "
          + ", ".join(f"gain {g:g}: {np.exp(t / n_rows):.3f}" for g, t in zip(GAINS, totals)))


if __name__ == "__main__":
    main()

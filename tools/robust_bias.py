#!/usr/bin/env python3
"""The error and the bias of the firefly-robust resolve (rene_resolve_robust) on the CPU oracle's renders: DESIGN.md section 4c's table.

For every scene, frame count and master seed (DEFAULT_SEED + 977 i, i = 0 .. 3): relMSE (tests/atrous_reference.py) of the plain mean and of the
robust mean -- the numpy restatement tests/robust_reference.py in fp64 on the oracle's chains -- against 1024 oracle frames from frame 100000
(default seed), and the energy kept (image mean over the reference's mean).  No GPU is used.

    python tools/robust_bias.py [--threads 8]
    python tools/robust_bias.py --spread     the restatement's own fp32-vs-fp64 spread of the tile sums on the cases of tests/test_gpu_robust.py
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import robust_reference as rr  # noqa: E402
from atrous_reference import relmse  # noqa: E402
from oracle import oracle  # noqa: E402
from rene_amd import abi, scenes  # noqa: E402

CASES = [("veach_mis(96, 54)", lambda: scenes.veach_mis(96, 54), (32, 128)),
         ("cornell_fog(64, 64)", lambda: scenes.cornell_fog(64, 64), (16, 64)),
         ("cornell_box(64, 64)", lambda: scenes.cornell_box(64, 64), (16, 64, 256))]
SEEDS = [abi.DEFAULT_SEED + 977 * i for i in range(4)]


SPREAD_CASES = [("cornell_box(100, 70) @ 12", lambda: scenes.cornell_box(100, 70), 12), ("cornell_box(100, 70) @ 5", lambda: scenes.cornell_box(100, 70), 5),
                ("cornell_fog(96, 64) @ 32", lambda: scenes.cornell_fog(96, 64), 32), ("veach_mis(96, 54) @ 32", lambda: scenes.veach_mis(96, 54), 32),
                ("dragon_class(240, 136) @ 16", lambda: scenes.dragon_class(240, 136), 16)]


def spread(threads):
    """max over tiles of |fp32 - fp64| / (|fp64| + the largest tile's value) for the two tile sums, the restatement run in either type on the
    oracle's chains; and the same with the fp32 run's own pixels summed in fp64 (no pixel differs in j between the two: rounding of the sums alone)."""
    for name, make, spp in SPREAD_CASES:
        o = oracle.Oracle(make())
        chains = np.zeros((8, o.yres, o.xres, 3), np.float32)
        for fr in range(spp):
            o.reset()
            o.render(fr, 1, threads=threads)
            chains[fr % 8] += o.download(0)
        n_c = rr.chain_counts(spp)
        r64, r32 = rr.resolve(chains, n_c), rr.resolve(chains, n_c, dtype=np.float32)
        t64 = rr.tile_records(r64["lum_plain"], r64["lum_robust"], r64["j"])
        t32 = rr.tile_records(r32["lum_plain"], r32["lum_robust"], r32["j"])
        s32 = rr.tile_records(r32["lum_plain"].astype(np.float64), r32["lum_robust"].astype(np.float64), r32["j"])
        rel = lambda x, y: float((np.abs(x.astype(np.float64) - y) / (np.abs(y) + np.abs(y).max())).max())
        print(f"{name}: pixels whose j differs between fp32 and fp64: {int((r64['j'] != r32['j']).sum())} of {r64['j'].size}; "
              f"fp32 vs fp64: sum_lum_plain {rel(t32[0], t64[0]):.3g}, sum_lum_robust {rel(t32[1], t64[1]):.3g}; "
              f"the fp32 pixels summed in fp32 vs in fp64: {rel(t32[0], s32[0]):.3g}, {rel(t32[1], s32[1]):.3g}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--spread", action="store_true")
    a = ap.parse_args()
    if a.spread:
        return spread(a.threads)
    print("| scene | frames | relMSE of the plain mean | relMSE robust | robust energy | pixels trimmed |")
    print("|---|---|---|---|---|---|")
    for name, make, marks in CASES:
        o = oracle.Oracle(make())
        o.render(100000, 1024, threads=a.threads)
        ref = o.download(0).astype(np.float64) / 1024
        rows = {m: [] for m in marks}
        for seed in SEEDS:
            chains = np.zeros((8, o.yres, o.xres, 3), np.float32)
            for fr in range(max(marks)):
                o.reset()
                o.render(fr, 1, seed=seed, threads=a.threads)
                chains[fr % 8] += o.download(0)
                if fr + 1 in marks:
                    out = rr.resolve(chains, rr.chain_counts(fr + 1))
                    rows[fr + 1].append((relmse(out["plain"], ref), relmse(out["image"], ref), float(out["image"].mean() / ref.mean()), float((out["j"] > 0).mean())))
        for m in marks:
            r = np.array(rows[m])
            rng = lambda c, fmt: f"{fmt % r[:, c].min()} – {fmt % r[:, c].max()}"
            print(f"| `{name}` | {m} | {rng(0, '%.3g')} (default seed {r[0, 0]:.3g}) | {rng(1, '%.3g')} ({r[0, 1]:.3g}) | {rng(2, '%.3f')} ({r[0, 2]:.3f}) | {rng(3, '%.2f')} |", flush=True)


if __name__ == "__main__":
    main()

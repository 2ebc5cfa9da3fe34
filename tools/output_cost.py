"""tools/output_cost.py [OUT.json]: what the output transform on the device costs.

cornell_box at 1920 x 1080 @ 16 frames and at 7680 x 4320 @ 8.  Kernel times: on ONE context rene_output_8bit (RGB8 and RGBA8, into tensors of the
caller's) and rene_download_mean alternate, 41 times each, a different one first in every round and each right behind one more rendered frame.  The yardstick is tile_mean_kernel, rene_download_mean's kernel, in the same session: it
reads the same 16 bytes per pixel and writes 16 where the output kernel writes 3 or 4.  The times are the library's own HIP events around its
launches (RENE_DEBUG=1 prints them per kernel): the measuring runs in a child process started with that variable, whose log this process reads.
End to end, in a second child without the variable: the wall time from a render that has been waited for to 8-bit pixels in host memory, through
Renderer.rgb8() and through download() + to_rgb8().  Medians and 10th - 90th percentiles, in ms.

tools/output_cost.py --tonemap [OUT.txt]: what exposure and a tone curve add (rene_output_tonemapped), and what the luminance histogram takes
(rene_luminance_histogram), at the same two sizes.  On one warm context the plain output_kernel<sRGB, RGB8>, the three tone-mapped kernels (RGB8,
+1 EV) and the histogram's two launches take turns, each behind one more rendered frame, a different one first in every round; the yardstick is
the plain kernel in the same run.  The child runs twice: the plain kernel's two medians and its 10th - 90th percentiles are the spread a ratio
has to exceed to mean anything.  Default output: profiles/tonemap_cost.txt."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 41
SIZES = ((1920, 1080, 16, 11), (7680, 4320, 8, 5))  # width, height, frames, end-to-end repetitions (the host path takes seconds at the larger size)


def child_kernels():
    from rene_amd import abi, api, scenes
    L = api.lib()
    for w, h, spp, _ in SIZES:
        with api.Renderer(scenes.cornell_box(w, h)) as r:
            r.render(0, spp)
            import torch
            dst = {abi.OUTPUT_RGB8: torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0"), abi.OUTPUT_RGBA8: torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")}
            torch.cuda.synchronize()
            mean = np.empty((h, w, 3), np.float32)

            def output(source, fmt):
                p = api.output_params_default()
                p.source, p.format = source, fmt
                t = dst[fmt]
                return lambda: api._check(L.rene_output_8bit(r._h, C.byref(p), C.c_void_p(t.data_ptr()), t.numel()))

            # rene_download_mean ends in a download and a repack on the host, during which the device idles and its clocks fall, and the kernel that
            # comes next pays for it.  So every timed call follows one more rendered frame, as the output stage of a job follows its render: the
            # call waits for the frame, resolves the image and launches its kernel on a device that has just been busy -- the same for all three
            done = [spp]

            def primer():
                r.render(done[0], 1)
                done[0] += 1

            calls = [output(abi.OUTPUT_RADIANCE, abi.OUTPUT_RGB8), output(abi.OUTPUT_RADIANCE, abi.OUTPUT_RGBA8),
                     lambda: api._check(L.rene_download_mean(r._h, 0, 3, mean.ctypes.data_as(C.c_void_p), mean.size))]
            rounds = [0]

            def one_round():  # the three in turn, a different one first every round
                for k in range(3):
                    primer()
                    calls[(k + rounds[0]) % 3]()
                rounds[0] += 1

            print("[cost] warm-up", file=sys.stderr, flush=True)
            for _ in range(3):  # allocations, code objects
                one_round()
            print(f"[cost] {w} {h} {spp}", file=sys.stderr, flush=True)
            for _ in range(REPS):
                one_round()


TONEMAP_REPS, TONEMAP_RUNS = 21, 2
TONEMAP_PATTERNS = {"output_kernel<sRGB, RGB8> (plain)": r"\[rene\] output .*, source 0, rgb8, ms: kernel (\S+)",
                    "tonemap_kernel<CLAMP, RGB8>": r"\[rene\] output .*, source 0, rgb8, clamp, .*ms: kernel (\S+)",
                    "tonemap_kernel<REINHARD, RGB8>": r"\[rene\] output .*, source 0, rgb8, reinhard, .*ms: kernel (\S+)",
                    "tonemap_kernel<ACES, RGB8>": r"\[rene\] output .*, source 0, rgb8, aces, .*ms: kernel (\S+)",
                    "luminance_kernel + luminance_sum_kernel": r"\[rene\] luminance histogram .*, ms: kernels (\S+)"}


def child_tonemap():
    from rene_amd import abi, api, scenes
    import torch
    L = api.lib()
    for w, h, spp, _ in SIZES:
        with api.Renderer(scenes.cornell_box(w, h)) as r:
            r.render(0, spp)
            t = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            plain = api.output_params_default()

            def tonemapped(op):
                p = api.tonemap_params_default()
                p.op, p.scale = op, api.exposure_scale(8)
                return lambda: api._check(L.rene_output_tonemapped(r._h, C.byref(p), C.c_void_p(t.data_ptr()), t.numel()))

            calls = [lambda: api._check(L.rene_output_8bit(r._h, C.byref(plain), C.c_void_p(t.data_ptr()), t.numel())),
                     tonemapped(abi.TONEMAP_CLAMP), tonemapped(abi.TONEMAP_REINHARD), tonemapped(abi.TONEMAP_ACES), lambda: r.luminance_stats()]
            done = spp
            for k in range(TONEMAP_REPS + 3):  # every call behind one more rendered frame (child_kernels has the reason), a different one first every round
                if k in (0, 3):
                    print("[cost] warm-up" if k == 0 else f"[cost] {w} {h} {spp}", file=sys.stderr, flush=True)
                for j in range(len(calls)):
                    r.render(done, 1)
                    done += 1
                    calls[(j + k) % len(calls)]()


def parse_log(text, patterns):
    kernels, section = {}, None
    for line in text.splitlines():
        if line.startswith("[cost] "):
            section = line[len("[cost] "):]
            kernels.setdefault(section, {})
            continue
        for name, pattern in patterns.items():
            m = re.match(pattern, line)
            if m and section is not None:
                kernels[section].setdefault(name, []).append(float(m.group(1)))
    kernels.pop("warm-up", None)
    return kernels


def main_tonemap(out_path):
    runs = []
    for _ in range(TONEMAP_RUNS):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tonemap-kernels"], env=dict(os.environ, RENE_DEBUG="1"), stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            sys.exit(p.returncode)
        runs.append(parse_log(p.stderr, TONEMAP_PATTERNS))
    yard = list(TONEMAP_PATTERNS)[0]
    lines = [f"tools/output_cost.py --tonemap: HIP events around the library's launches, ms; {TONEMAP_REPS} launches per kernel and run, {TONEMAP_RUNS} runs (processes)",
             "ratio: a kernel's median over the plain output kernel's median of the same run", ""]
    for section in runs[0]:
        lines.append(f"cornell_box, width height frames = {section}")
        for name in TONEMAP_PATTERNS:
            for k, run in enumerate(runs):
                f, y = figures(run[section][name]), figures(run[section][yard])
                lines.append(f"  run {k}  {name:42s} median {f['median']:.4f}  p10 {f['p10']:.4f}  p90 {f['p90']:.4f}  n {f['n']}  ratio {f['median'] / y['median']:.3f}")
        y = [figures(run[section][yard]) for run in runs]
        lines.append(f"  spread of the plain kernel: medians {min(v['median'] for v in y):.4f} .. {max(v['median'] for v in y):.4f} across runs "
                     f"({max(v['median'] for v in y) / min(v['median'] for v in y):.3f}); p90 / p10 within a run {max(v['p90'] / v['p10'] for v in y):.3f}")
        lines.append("")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))


def child_end_to_end():
    from rene_amd import api, scenes
    result = {}
    for w, h, spp, reps in SIZES:
        with api.Renderer(scenes.cornell_box(w, h)) as r:
            r.render(0, spp)
            r.sync()
            paths = {"device: Renderer.rgb8()": lambda: r.rgb8(), "host: download() + to_rgb8()": lambda: api.to_rgb8(r.download(0), spp)}
            images = {name: f() for name, f in paths.items()}  # warm-up: allocations, pinned staging
            assert np.array_equal(*images.values())
            times = {name: [] for name in paths}
            for _ in range(reps):
                for name, f in paths.items():
                    r.sync()
                    t0 = time.perf_counter()
                    f()
                    times[name].append(1e3 * (time.perf_counter() - t0))
            result[f"{w} {h} {spp}"] = times
    print(json.dumps(result))


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "output_cost.json")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels"], env=dict(os.environ, RENE_DEBUG="1"), stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    patterns = {"output_kernel, sRGB, RGB8": r"\[rene\] output .*, source 0, rgb8, ms: kernel (\S+)",
                "output_kernel, sRGB, RGBA8": r"\[rene\] output .*, source 0, rgba8, ms: kernel (\S+)",
                "tile_mean_kernel (rene_download_mean)": r"\[rene\] download_mean .*, ms: kernel (\S+)"}
    kernels, section = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[cost] "):
            section = line[len("[cost] "):]
            kernels[section] = {}
            continue
        for name, pattern in patterns.items():
            m = re.match(pattern, line)
            if m and section is not None:
                kernels[section].setdefault(name, []).append(float(m.group(1)))
    kernels.pop("warm-up", None)
    for section, ks in kernels.items():
        for name, values in ks.items():
            ks[name] = f = figures(values)
            print(f"{section:16s} {name:44s} median {f['median']:.4f} ms (p10 {f['p10']:.4f}, p90 {f['p90']:.4f}, n {f['n']})")
        yard = ks["tile_mean_kernel (rene_download_mean)"]["median"]
        for name in list(ks)[:2]:
            print(f"{section:16s} {name} / tile_mean_kernel: {ks[name]['median'] / yard:.3f}")
    env = {k: v for k, v in os.environ.items() if k != "RENE_DEBUG"}
    q = subprocess.run([sys.executable, os.path.abspath(__file__), "--end-to-end"], env=env, stdout=subprocess.PIPE, text=True)
    if q.returncode != 0:
        sys.exit(q.returncode)
    end_to_end = json.loads(q.stdout.strip().splitlines()[-1])
    for section, paths in end_to_end.items():
        for name, values in paths.items():
            paths[name] = f = figures(values)
            print(f"{section:16s} {name:44s} median {f['median']:.2f} ms (p10 {f['p10']:.2f}, p90 {f['p90']:.2f}, n {f['n']})")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms", "kernels": {"what": "HIP events around the library's launches", "reps": REPS, "results": kernels},
                   "end_to_end": {"what": "wall time from a render that has been waited for to 8-bit pixels in host memory", "results": end_to_end}}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if "--kernels" in sys.argv:
        child_kernels()
    elif "--tonemap-kernels" in sys.argv:
        child_tonemap()
    elif "--tonemap" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--tonemap"]
        main_tonemap(rest[0] if rest else os.path.join(ROOT, "profiles", "tonemap_cost.txt"))
    elif "--end-to-end" in sys.argv:
        child_end_to_end()
    else:
        main()

"""tools/exr_cost.py [OUT.json] [--kernels-only]: what the multi-channel OpenEXR output on the device costs.

One process, cornell_box at 1920 x 1080 @ 16 frames with the geometry pass over those frames and the a-trous denoiser behind them.
Kernel times: on ONE context rene_output_exr with BEAUTY alone and with every layer (into tensors of the caller's) and rene_output_8bit RGBA8, the
yardstick, take turns 21 times, a different one first in every round and each right behind one more rendered frame (tools/output_cost.py has the
reason).  The times are the library's own HIP events around its launches, which RENE_DEBUG=1 prints per kernel: the variable is set for that
phase and the process's stderr goes to a file, which is read back.  Next to every time: the bytes the kernel reads plus the bytes it writes,
counted from the shapes, over that time.
End to end, without the variable, 21 alternating runs: the wall time from a context that has been waited for to the FILE'S BYTES in host memory --
through Renderer.exr() with every layer, and by the route of a build without the call: download_mean x 3, download_denoised(MEAN), the records of
the geometry pass and a numpy pack.  The two files are compared byte for byte before anything is timed.
Medians and 10th - 90th percentiles, in ms.  --kernels-only: the first phase alone, its figures as one JSON line on stdout (A/B of library
variants: RENE_HIP_LIB=librene_hip_NAME.so)."""
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 21
W, H, SPP = 1920, 1080, 16


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def numpy_body(abi, mask, planes):
    """The body as one structured array, a record per scan line: the two prefix ints, then every channel's row."""
    types = {"half": "<f2", "float": "<f4", "uint": "<u4"}
    chans = [(n, types[t]) for n, b, t in abi.EXR_CHANNELS if mask & b]
    rows = np.zeros(H, np.dtype([("y", "<i4"), ("size", "<i4")] + [(n, dt, (W,)) for n, dt in chans]))
    rows["y"] = np.arange(H)
    rows["size"] = sum(np.dtype(dt).itemsize for _, dt in chans) * W
    for n, dt in chans:
        a = planes[n]
        if dt == "<f2":
            with np.errstate(invalid="ignore", over="ignore"):
                a = np.where(a > 65504, np.float32(65504), np.where(a < -65504, np.float32(-65504), a))
        rows[n] = a.astype(dt)
    return rows.tobytes()


def parent_route(abi, api, r, mask):
    """The file's bytes by the route of a build without rene_output_exr: five downloads and a pack on the host."""
    mean = [r.download_mean(l) for l in range(3)]
    dn = r.download_denoised(abi.DENOISED_MEAN)
    rec = api._download_result(r, api.lib().rene_download_gbuffer, (H, W), abi.GBUFFER_DTYPE)
    hits, n = rec["hits"].astype(np.float32), rec["n"].astype(np.float32)
    planes = {}
    for k, c in enumerate("RGB"):
        planes[c], planes["albedo." + c], planes["denoised." + c] = mean[0][..., k], mean[2][..., k], dn[..., k]
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, c in enumerate("XYZ"):
            planes["normal." + c] = mean[1][..., k]
            planes["P." + c] = np.where(rec["hits"] > 0, rec["position_sum"][..., k] / hits, np.float32(0))
        planes["A"] = np.where(rec["n"] > 0, hits / n, np.float32(0))
        planes["Z"] = np.where(rec["hits"] > 0, rec["depth_sum"] / hits, np.float32(np.inf))
        for k in range(4):
            planes[f"id{k}"] = rec["id"][..., k]
            planes[f"cov{k}"] = np.where(rec["n"] > 0, rec["count"][..., k].astype(np.float32) / n, np.float32(0))
    return api.exr_header(W, H, mask) + numpy_body(abi, mask, planes)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels-only" in sys.argv
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "exr_cost.json")
    from rene_amd import abi, api, scenes
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/exr_cost.py measures on the GPU and there is none")
    L = api.lib()
    masks = {"exr_kernel, BEAUTY": abi.EXR_BEAUTY, "exr_kernel, every layer": abi.EXR_ALL}
    n_px = W * H
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.render(0, SPP)
        r.gbuffer(0, SPP)
        r.denoise()
        dst = {name: torch.empty((api.exr_layout(W, H, m)[1],), dtype=torch.uint8, device="cuda:0") for name, m in masks.items()}
        rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def exr(name):
            p = api._exr_params(masks[name], "radiance")
            t = dst[name]
            return lambda: api._check(L.rene_output_exr(r._h, C.byref(p), C.c_void_p(t.data_ptr()), t.numel()))

        p8 = api.output_params_default()
        p8.format = abi.OUTPUT_RGBA8
        calls = [exr("exr_kernel, BEAUTY"), exr("exr_kernel, every layer"), lambda: api._check(L.rene_output_8bit(r._h, C.byref(p8), C.c_void_p(rgba.data_ptr()), rgba.numel()))]
        patterns = {"exr_kernel, BEAUTY": r"\[rene\] exr body .*, layers 0x01, .*ms: kernel (\S+)", "exr_kernel, every layer": r"\[rene\] exr body .*, layers 0xff, .*ms: kernel (\S+)",
                    "output_kernel, sRGB, RGBA8": r"\[rene\] output .*, source 0, rgba8, ms: kernel (\S+)"}
        # bytes read + written per launch, from the shapes: 16 per pixel and image layer, 64 per record, 4 per tile's count (not counted: 2040 tiles)
        moved = {"exr_kernel, BEAUTY": n_px * 16 + dst["exr_kernel, BEAUTY"].numel(), "exr_kernel, every layer": n_px * (4 * 16 + 64) + dst["exr_kernel, every layer"].numel(),
                 "output_kernel, sRGB, RGBA8": n_px * (16 + 4)}
        done = SPP
        log = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["RENE_DEBUG"] = "1"
        try:
            os.dup2(log.fileno(), 2)
            for k in range(REPS + 3):  # three rounds of warm-up: allocations, code objects
                if k == 3:
                    os.write(2, b"[cost] measured\n")
                for j in range(len(calls)):
                    r.render(done, 1)
                    done += 1
                    calls[(j + k) % len(calls)]()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["RENE_DEBUG"]
        log.seek(0)
        text = log.read().decode(errors="replace")
        text = text[text.index("[cost] measured"):]
        kernels = {}
        for name, pattern in patterns.items():
            f = figures([float(m.group(1)) for m in re.finditer(pattern, text)])
            assert f["n"] == REPS, (name, f)
            f["bytes_moved"] = int(moved[name])
            f["GB_per_s"] = round(moved[name] / (f["median"] * 1e-3) / 1e9, 1)
            kernels[name] = f
            print(f"{name:32s} median {f['median']:.4f} ms (p10 {f['p10']:.4f}, p90 {f['p90']:.4f}, n {f['n']}), {moved[name]} bytes read + written, {f['GB_per_s']} GB/s", file=sys.stderr)
        if kernels_only:
            print(json.dumps({"lib": os.environ.get("RENE_HIP_LIB", "librene_hip.so"), "kernels": kernels}))
            return
        mask = abi.EXR_ALL
        routes = {"device: Renderer.exr(), every layer": lambda: r.exr(layers=mask), "host: 3 x download_mean, download_denoised, the records, numpy pack": lambda: parent_route(abi, api, r, mask)}
        files = {name: f() for name, f in routes.items()}  # warm-up: allocations, pinned staging
        a, b = files.values()
        assert a == b, "the two routes write different files"
        times = {name: [] for name in routes}
        for _ in range(REPS):
            for name, f in routes.items():
                r.sync()
                t0 = time.perf_counter()
                f()
                times[name].append(1e3 * (time.perf_counter() - t0))
        end_to_end = {}
        for name, v in times.items():
            end_to_end[name] = f = figures(v)
            print(f"{name:72s} median {f['median']:.2f} ms (p10 {f['p10']:.2f}, p90 {f['p90']:.2f}, n {f['n']})", file=sys.stderr)
        bpp = api.exr_layout(W, H, mask)[2]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"command": "python tools/exr_cost.py", "scene": f"cornell_box {W} x {H} @ {SPP} frames", "unit": "ms",
                   "kernels": {"what": "HIP events around the library's launches of the kernel named (the denoised mean's own launch ahead of exr_kernel is not in them); "
                                       "bytes_moved: read + written, from the shapes", "reps": REPS, "results": kernels},
                   "end_to_end": {"what": "wall time from a context that has been waited for to the file's bytes in host memory; the two files are equal byte for byte",
                                  "file_bytes": len(a), "pcie_bytes_per_pixel": {"device": bpp, "host": 128}, "reps": REPS, "results": end_to_end}}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

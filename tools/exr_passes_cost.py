"""tools/exr_passes_cost.py [OUT.json] [--ab LIB.so]: what the pass-layer OpenEXR output costs on the device.  Recorded, not gated.

One MI355X, one process; cornell_box at 1920 x 1080, 8 frames rendered, the occlusion, direct-light, bounce and light-group passes over frames 0 .. 7
in the library's buffers.  Recorded: the pack kernel's time (exr_passes_kernel, the library's own HIP events: RENE_DEBUG=1 prints them) for `ao`
alone and for every layer, beside exr_kernel packing RENE_EXR_ALL in the SAME run, the three calls taking turns, 21 rounds after 3 warm-ups -- each
also per byte read + written, exr_kernel's figure being the yardstick; the wall time from a context that has been waited for to the file's bytes in
host memory, uncompressed and ZIPS, against the route without the pack (four record downloads, the api.* reductions, a numpy pack); the file's
bytes and the ZIPS ratio.  --ab LIB.so: the kernel times once more in a fresh child process under RENE_HIP_LIB=LIB.so (a build of another load
schedule, Makefile `variant`), with its own exr_kernel yardstick.  Medians and 10th - 90th percentiles, in ms."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 21
W, H, FRAMES = 1920, 1080, 8
# bytes a lane reads + writes: the records' and the radiance's in, the halves out (exr_kernel: four [4] float layers, the 64-byte record; 66 out)
TRAFFIC = {"ao": 16 + 2, "all": 32 + 48 + 176 + 144 + 16 + 130, "exr_all": 4 * 16 + 64 + 66}


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def prepare(api, scenes):
    r = api.Renderer(scenes.cornell_box(W, H))
    r.render(0, FRAMES)
    for run in (r.occlusion, r.direct, r.bounces, r.lights):
        run(0, FRAMES)
    r.gbuffer(0, FRAMES)
    r.denoise()
    return r


def kernel_times(api, abi, r):
    ao, _ = api._exr_passes_params("ao", None, None)
    every, _ = api._exr_passes_params(abi.EXRP_ALL, None, None)
    exr = api._exr_params(abi.EXR_ALL, "radiance")
    L = api.lib()
    calls = [lambda: api._check(L.rene_output_exr_passes(r._h, C.byref(ao), None, 0)), lambda: api._check(L.rene_output_exr_passes(r._h, C.byref(every), None, 0)),
             lambda: api._check(L.rene_output_exr(r._h, C.byref(exr), None, 0))]
    log = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    saved = os.dup(2)
    os.environ["RENE_DEBUG"] = "1"
    try:
        os.dup2(log.fileno(), 2)
        for k in range(REPS + 3):  # three rounds of warm-up
            if k == 3:
                os.write(2, b"[cost] measured\n")
            for j in range(3):
                calls[(j + k) % 3]()
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        del os.environ["RENE_DEBUG"]
    log.seek(0)
    text = log.read().decode(errors="replace")
    text = text[text.index("[cost] measured"):]
    t = {"ao": [float(m.group(1)) for m in re.finditer(r"\[rene\] exr passes body .*layers 0x01, .*ms: kernel (\S+)", text)],
         "all": [float(m.group(1)) for m in re.finditer(r"\[rene\] exr passes body .*layers 0x7f, .*ms: kernel (\S+)", text)],
         "exr_all": [float(m.group(1)) for m in re.finditer(r"\[rene\] exr body .*layers 0xff, .*ms: kernel (\S+)", text)]}
    assert all(len(v) == REPS for v in t.values()), {k: len(v) for k, v in t.items()}
    out = {"exr_passes_kernel, ao": figures(t["ao"]), "exr_passes_kernel, every layer": figures(t["all"]), "exr_kernel, RENE_EXR_ALL": figures(t["exr_all"]),
           "bytes_read_and_written_per_pixel": TRAFFIC}
    ps = {k: 1e9 * float(np.median(v)) / (W * H * TRAFFIC[k]) for k, v in t.items()}  # ms -> ps per byte
    out["ps_per_byte"] = {k: round(v, 4) for k, v in ps.items()}
    out["over_exr_kernel_per_byte"] = {"ao": round(ps["ao"] / ps["exr_all"], 4), "all": round(ps["all"] / ps["exr_all"], 4)}
    e = out["exr_kernel, RENE_EXR_ALL"]
    out["exr_kernel_spread_p90_over_p10"] = round(e["p90"] / e["p10"], 4)
    return out


def numpy_route(api, abi, r):
    """What users have without the pack: the four record downloads, the api.* reductions, a numpy pack of the same body.  For TIMING only: the
    halves are a plain clamp and cast, without the file's 0x7e00 rule for NaNs, and main() compares one channel row with the device's -- the
    parity checks are tests/test_gpu_exr_passes.py's."""
    L = api.lib()
    rec = {n: api._download_result(r, getattr(L, "rene_download_" + n), (H, W), np.dtype(getattr(abi, n.upper() + "_DTYPE"))) for n in ("occlusion", "direct", "bounces", "lights")}
    beauty = r.download(0)
    planes = {"ao": api.occlusion_ao(rec["occlusion"]), "pathlength": api.bounces_mean_length(rec["bounces"])}
    with np.errstate(all="ignore"):
        for stem, img, names in [("bent", api.occlusion_bent(rec["occlusion"]), "XYZ"), ("direct", api.direct_mean(rec["direct"]), "RGB"),
                                 ("indirect", api.indirect_mean(beauty, rec["direct"]), "RGB")] + \
                                [(f"depth{d}", api.bounces_depth_mean(rec["bounces"], d), "RGB") for d in range(10)] + \
                                [(f"light{g}", api.lights_group_mean(rec["lights"], g), "RGB") for g in range(8)]:
            for k, c in enumerate(names):
                planes[f"{stem}.{c}"] = img[..., k]
        order = sorted(planes, key=lambda s: s.encode())
        body = np.empty((H, 8 + 2 * W * len(order)), np.uint8)
        body[:, :8] = np.stack([np.arange(H, dtype="<i4"), np.full(H, 2 * W * len(order), "<i4")], 1).view(np.uint8)
        for k, name in enumerate(order):
            half = np.clip(planes[name], -65504.0, 65504.0).astype("<f2")
            body[:, 8 + 2 * W * k:8 + 2 * W * (k + 1)] = half.view(np.uint8).reshape(H, 2 * W)
    return body.tobytes()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ab = sys.argv[sys.argv.index("--ab") + 1] if "--ab" in sys.argv else None
    if ab in args:
        args.remove(ab)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "exr_passes_cost.json")
    from rene_amd import abi, api, scenes
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/exr_passes_cost.py measures on the GPU and there is none")
    r = prepare(api, scenes)
    if "--kernels-only" in sys.argv:  # the child of --ab: its figures on stdout
        print(json.dumps(kernel_times(api, abi, r)))
        r.close()
        return
    kernels = kernel_times(api, abi, r)
    plain = r.exr_passes(compression="none")
    packed = r.exr_passes(compression="zips")
    sizes = {"file_bytes_uncompressed": len(plain), "file_bytes_zips": len(packed), "ratio": round(len(packed) / len(plain), 4),
             "record_bytes_downloaded_without_the_pack": W * H * (32 + 48 + 176 + 144 + 12)}
    routes = {"uncompressed": lambda: r.exr_passes(compression="none"), "zips": lambda: r.exr_passes(compression="zips"),
              "downloads + api reductions + numpy pack": lambda: numpy_route(api, abi, r)}
    assert numpy_route(api, abi, r)[:8 + 2 * W] == plain[-H * (8 + 130 * W):][:8 + 2 * W]  # (the same body: its first channel row)
    times = {name: [] for name in routes}
    for k in range(REPS + 1):  # one round of warm-up
        for name, f in routes.items():
            if name.startswith("downloads") and k > 5:  # (seconds per call: five rounds of it)
                continue
            r.sync()
            t0 = time.perf_counter()
            f()
            if k:
                times[name].append(1e3 * (time.perf_counter() - t0))
    r.close()
    result = {"kernels": kernels, "sizes": sizes, "context_to_file_bytes": {name: figures(v) for name, v in times.items()}}
    if ab:  # a fresh child process: another build of the library, the same protocol
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only"], env=dict(os.environ, RENE_HIP_LIB=ab), capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            sys.exit("the --ab child failed:\n" + child.stderr[-2000:])
        result["ab"] = {"library": ab, "kernels": json.loads(child.stdout.strip().splitlines()[-1])}
    print(json.dumps(result), file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"command": "python tools/exr_passes_cost.py" + (f" --ab {ab}" if ab else ""), "film": f"cornell_box {W} x {H} @ {FRAMES} frames, the four passes over frames 0 .. 7",
                   "unit": "ms", "reps": REPS,
                   "what": "kernels: HIP events around the library's launches, the three calls taking turns; ps_per_byte: the median over bytes read + written; "
                           "context_to_file_bytes: wall time of Renderer.exr_passes() -- pack, compression, download -- against four record downloads, the api.* "
                           "reductions and a numpy pack, the routes alternating; ab: the kernel times of another build of the library in a child process",
                   "results": result}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

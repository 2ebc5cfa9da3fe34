"""tools/cryptomatte_cost.py [OUT.json]: what the Cryptomatte output costs on the device.  Recorded, not gated.

One process; cornell_box and dragon_class at 1920 x 1080, the geometry pass over 16 frames, the two layers CryptoObject and CryptoMaterial.
Recorded per scene: the pack kernel's time (cryptomatte_kernel, the library's own HIP events: RENE_DEBUG=1 prints them) beside exr_kernel packing
IDS | DEPTH | POSITION -- its 4-byte-channel case, from the same records -- both also per byte of body written, 21 rounds, the two calls taking turns;
the file's bytes uncompressed and as ZIPS; the wall time from a context that has been waited for to the file's bytes in host memory
(Renderer.cryptomatte: two geometry passes, the pack, the compression, the download), compressed and uncompressed, alternating in the same run.
Medians and 10th - 90th percentiles, in ms."""
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
W, H, FRAMES = 1920, 1080, 16


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "cryptomatte_cost.json")
    from rene_amd import abi, api, scenes
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/cryptomatte_cost.py measures on the GPU and there is none")
    exr_mask = abi.EXR_IDS | abi.EXR_DEPTH | abi.EXR_POSITION
    exr_body = api.exr_layout(W, H, exr_mask)[1]
    results = {}
    for scene_name, build in (("cornell_box", scenes.cornell_box), ("dragon_class", scenes.dragon_class)):
        scene = build(W, H)
        with api.Renderer(scene) as r:
            layers = api.cryptomatte_scene_layers(("object", "material"), lambda layer: api._cryptomatte_names(r, layer, None))
            body = api.cryptomatte_layout(W, H, layers)[1]
            plain = r.cryptomatte(n_frames=FRAMES, compression="none")
            packed = r.cryptomatte(n_frames=FRAMES, compression="zips")
            sizes = {"file_bytes_uncompressed": len(plain), "file_bytes_zips": len(packed), "ratio": round(len(packed) / len(plain), 4)}
            # kernel times: the library's events.  The material records in a tensor, the instance records in the library's buffer, as cryptomatte() leaves them
            rec = torch.empty(api.gbuffer_bytes(W, H), dtype=torch.uint8, device=f"cuda:{r.device}")
            r.gbuffer_into(rec, 0, FRAMES, "material")
            r.gbuffer(0, FRAMES, "instance")
            full = [layers[0] + (None,), layers[1] + (rec,)]
            p = api._exr_params(exr_mask, "radiance")
            calls = [lambda: r.output_cryptomatte(full, download=False), lambda: api._check(api.lib().rene_output_exr(r._h, C.byref(p), None, 0))]
            log = tempfile.TemporaryFile(mode="w+b")
            sys.stderr.flush()
            saved = os.dup(2)
            os.environ["RENE_DEBUG"] = "1"
            try:
                os.dup2(log.fileno(), 2)
                for k in range(REPS + 3):  # three rounds of warm-up
                    if k == 3:
                        os.write(2, b"[cost] measured\n")
                    for j in range(2):
                        calls[(j + k) % 2]()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
                del os.environ["RENE_DEBUG"]
            log.seek(0)
            text = log.read().decode(errors="replace")
            text = text[text.index("[cost] measured"):]
            pack = [float(m.group(1)) for m in re.finditer(r"\[rene\] cryptomatte body .*ms: kernel (\S+)", text)]
            exr = [float(m.group(1)) for m in re.finditer(rf"\[rene\] exr body .*, layers 0x{exr_mask:02x}, .*ms: kernel (\S+)", text)]
            assert len(pack) == REPS and len(exr) == REPS, (len(pack), len(exr))
            kernels = {"cryptomatte_kernel, 2 layers": figures(pack), "exr_kernel, IDS | DEPTH | POSITION": figures(exr),
                       "body_bytes": {"cryptomatte": body, "exr": exr_body},
                       "ns_per_byte": {"cryptomatte": round(1e6 * float(np.median(pack)) / body, 6), "exr": round(1e6 * float(np.median(exr)) / exr_body, 6)}}
            kernels["cryptomatte_over_exr_per_byte"] = round(kernels["ns_per_byte"]["cryptomatte"] / kernels["ns_per_byte"]["exr"], 4)
            # context to file bytes
            routes = {"uncompressed": lambda: r.cryptomatte(n_frames=FRAMES, compression="none"), "zips": lambda: r.cryptomatte(n_frames=FRAMES, compression="zips")}
            times = {name: [] for name in routes}
            for _ in range(REPS):
                for name, f in routes.items():
                    r.sync()
                    t0 = time.perf_counter()
                    f()
                    times[name].append(1e3 * (time.perf_counter() - t0))
            results[scene_name] = {"instances": len(scene.instances), "materials": len(scene.materials), "sizes": sizes, "kernels": kernels,
                                   "context_to_file_bytes": {name: figures(v) for name, v in times.items()}}
            print(scene_name, json.dumps(results[scene_name]), file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"command": "python tools/cryptomatte_cost.py", "film": f"{W} x {H} @ {FRAMES} frames, CryptoObject and CryptoMaterial", "unit": "ms", "reps": REPS,
                   "what": "kernels: HIP events around the library's launches, the two calls taking turns; ns_per_byte: the median over the body's bytes; "
                           "context_to_file_bytes: wall time of Renderer.cryptomatte() -- two geometry passes, pack, compression, download -- the two routes alternating",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

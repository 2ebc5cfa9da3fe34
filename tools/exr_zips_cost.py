"""tools/exr_zips_cost.py [OUT.json]: what the ZIPS compression of the OpenEXR output on the device gives and costs.

One process, tools/exr_cost.py's workload: cornell_box at 1920 x 1080 @ 16 frames with the geometry pass over those frames and the a-trous denoiser
behind them; BEAUTY alone and every layer.
Recorded per layer set: the file's bytes compressed and uncompressed; the share of rows stored raw; the bytes zlib.compress level 6 gives for the same
pre-processed rows, one stream per row, computed on the host -- the yardstick for what dynamic codes and real matching would add; the library's
own HIP events around the size, scan and encode kernels and around exr_kernel (RENE_DEBUG=1 prints them; tools/exr_cost.py has the method), 21
rounds, the calls taking turns, each behind one more rendered frame.
Gated, every layer: the wall time from a context that has been waited for to the file's bytes in host memory, Renderer.exr(compression="zips")
against the uncompressed Renderer.exr(), 21 rounds, the two alternating in the same run.  The compressed median must not exceed the uncompressed
median x (1 + s), s = (p90 - p10) / median of the uncompressed series.  Medians and 10th - 90th percentiles, in ms."""
import json
import os
import re
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 21
W, H, SPP = 1920, 1080, 16


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def zlib_yardstick(body, n):
    """The bytes of zlib.compress(level 6) over every row's pre-processed bytes, a row stored raw where that is no smaller: the chunks' data alone."""
    rows = np.frombuffer(body, np.uint8).reshape(H, 8 + n)[:, 8:]
    t = np.concatenate([rows[:, 0::2], rows[:, 1::2]], axis=1).astype(np.int16)
    d = t.copy()
    d[:, 1:] = (t[:, 1:] - t[:, :-1] + 128) % 256
    d = d.astype(np.uint8)
    return int(sum(min(n, len(zlib.compress(d[y].tobytes(), 6))) for y in range(H)))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "exr_zips_cost.json")
    from rene_amd import abi, api, scenes
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/exr_zips_cost.py measures on the GPU and there is none")
    masks = {"BEAUTY": abi.EXR_BEAUTY, "every layer": abi.EXR_ALL}
    sizes, kernels = {}, {}
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.render(0, SPP)
        r.gbuffer(0, SPP)
        r.denoise()
        for name, mask in masks.items():
            plain = r.exr(layers=mask)
            packed = r.exr(layers=mask, compression="zips")
            head, body_bytes, bpp = api.exr_layout(W, H, mask)
            n, attr = W * bpp, head - 8 * H
            assert api.exr_attributes(W, H, mask, "zips") + api.exr_compress_host(W, H, mask, plain[head:], "zips") == packed, "the device's file is not the host's"
            chunk_sizes, at = [], attr + 8 * H
            for y in range(H):
                assert struct.unpack_from("<Q", packed, attr + 8 * y)[0] == at
                chunk_sizes.append(struct.unpack_from("<i", packed, at + 4)[0])
                at += 8 + chunk_sizes[-1]
            assert at == len(packed)
            data = sum(chunk_sizes)
            yard = zlib_yardstick(plain[head:], n)
            sizes[name] = {"file_bytes_uncompressed": len(plain), "file_bytes_zips": len(packed), "ratio": round(len(packed) / len(plain), 4),
                           "rows": H, "rows_stored_raw": int(sum(s == n for s in chunk_sizes)), "chunk_data_bytes_zips": int(data),
                           "chunk_data_bytes_zlib_level_6": yard, "zlib_level_6_over_zips": round(yard / data, 4)}
            print(name, sizes[name], file=sys.stderr)
        # kernel times: the library's events
        done = SPP
        calls = [(name, comp) for name in masks for comp in ("none", "zips")]
        log = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["RENE_DEBUG"] = "1"
        try:
            os.dup2(log.fileno(), 2)
            for k in range(REPS + 3):  # three rounds of warm-up
                if k == 3:
                    os.write(2, b"[cost] measured\n")
                for j in range(len(calls)):
                    r.render(done, 1)
                    done += 1
                    name, comp = calls[(j + k) % len(calls)]
                    r.exr(layers=masks[name], compression=comp)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["RENE_DEBUG"]
        log.seek(0)
        text = log.read().decode(errors="replace")
        text = text[text.index("[cost] measured"):]
        for name, mask in masks.items():
            body = [float(m.group(1)) for m in re.finditer(rf"\[rene\] exr body .*, layers 0x{mask:02x}, .*ms: kernel (\S+)", text)]
            assert len(body) == 2 * REPS, (name, len(body))  # (either call packs the body first)
            kernels[f"exr_kernel, {name}"] = figures(body)
            z = [tuple(float(x) for x in m.groups()) for m in re.finditer(rf"\[rene\] exr zips .*, layers 0x{mask:02x}, .*ms: size (\S+) scan (\S+) encode (\S+)", text)]
            assert len(z) == REPS, (name, len(z))
            for k, part in enumerate(("zips_size_kernel", "zips_scan_kernel", "zips_encode_kernel")):
                kernels[f"{part}, {name}"] = figures([v[k] for v in z])
        for name, f in kernels.items():
            print(f"{name:40s} median {f['median']:.4f} ms (p10 {f['p10']:.4f}, p90 {f['p90']:.4f}, n {f['n']})", file=sys.stderr)
        # the gate: context to file bytes in host memory, every layer
        mask = abi.EXR_ALL
        routes = {"uncompressed: Renderer.exr(), every layer": lambda: r.exr(layers=mask), "zips: Renderer.exr(compression='zips'), every layer": lambda: r.exr(layers=mask, compression="zips")}
        for f in routes.values():
            f()
        times = {name: [] for name in routes}
        for _ in range(REPS):
            for name, f in routes.items():
                r.sync()
                t0 = time.perf_counter()
                f()
                times[name].append(1e3 * (time.perf_counter() - t0))
        end_to_end = {name: figures(v) for name, v in times.items()}
        for name, f in end_to_end.items():
            print(f"{name:56s} median {f['median']:.2f} ms (p10 {f['p10']:.2f}, p90 {f['p90']:.2f}, n {f['n']})", file=sys.stderr)
    base, comp = end_to_end.values()
    s = (base["p90"] - base["p10"]) / base["median"]
    gate = {"what": "zips median <= uncompressed median x (1 + s), s = (p90 - p10) / median of the uncompressed series of this run", "s": round(s, 4),
            "limit_ms": round(base["median"] * (1 + s), 4), "zips_over_uncompressed": round(comp["median"] / base["median"], 4), "met": bool(comp["median"] <= base["median"] * (1 + s))}
    print("gate", gate, file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"command": "python tools/exr_zips_cost.py", "scene": f"cornell_box {W} x {H} @ {SPP} frames", "unit": "ms",
                   "sizes": {"what": "the files of one job, compressed on the device (equal to the host's rene_exr_compress_host byte for byte) and uncompressed; "
                                     "chunk_data: the chunks' bytes without their 8-byte prefixes; zlib level 6: one stream per pre-processed row, on the host", "results": sizes},
                   "kernels": {"what": "HIP events around the library's launches of the kernel named", "reps": REPS, "results": kernels},
                   "end_to_end": {"what": "wall time from a context that has been waited for to the file's bytes in host memory, the two routes alternating", "reps": REPS,
                                  "results": end_to_end, "gate": gate}}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

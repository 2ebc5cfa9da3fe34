"""tools/state_cost.py [OUT.json] [--parent-lib PATH]: what saving and restoring a job's state costs.

cornell_box at 1920 x 1080 and 3840 x 2160, 8 frames.  Per size, in one process and on one warm context pair (a source that holds the frames, a
destination that is reset before every restore): the wall time of rene_save_state and of rene_restore_state -- into and from PINNED host memory,
which the copy engine reaches without a staging, and into and from pageable memory, which goes through the library's two stagings -- and, as the
yardstick, a bare copy of the same byte count between one device buffer and one pinned host buffer, in the same direction.  One warm-up round, then
REPS timed rounds in which the measurements take turns; medians and ranges (minimum - maximum), in ms.  The kernels' time is the library's own: HIP
events on either side of every chunk's kernel, summed (RENE_DEBUG=1 prints them).  Those events sit in the pipeline they time, so the measuring
runs in two child processes: one without the variable, from which the wall times are taken, and one with it, from which only the kernels' sums
and the pipeline's time under the events are taken (the keys that name them).

--parent-lib PATH: also rene_create on dragon_class() with this build's library and with the library at PATH (a build of the parent commit), three
alternating child processes each, five timed creates per child after one warm-up: what taking the scene's fingerprint costs at create.

Default output: profiles/state_cost.json."""
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
REPS = 7
SIZES = ((1920, 1080), (3840, 2160))
FRAMES = 8


def child_state():
    import torch
    from rene_amd import api, scenes
    for w, h in SIZES:
        s = scenes.cornell_box(w, h)
        n = api.state_bytes(w, h)
        with api.Renderer(s) as src, api.Renderer(s) as dst:
            src.render(0, FRAMES)
            src.sync()
            pinned = torch.empty(n, dtype=torch.uint8).pin_memory()
            pin = pinned.numpy()
            page = np.empty(n, np.uint8)
            dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()

            def timed(label, f):
                t0 = time.perf_counter()
                f()
                ms = (time.perf_counter() - t0) * 1e3
                print(f"[cost] {label} {ms:.4f}", file=sys.stderr, flush=True)

            def copy(to, frm):
                to.copy_(frm, non_blocking=True)
                torch.cuda.synchronize()

            def restore(blob):
                dst.reset()
                timed("restore " + ("pinned" if blob is pin else "pageable"), lambda: dst.restore_state(blob))

            for rep in range(REPS + 1):
                print(f"[cost] {'warm-up' if rep == 0 else 'round'} {w} {h} {n}", file=sys.stderr, flush=True)
                timed("copy d2h", lambda: copy(pinned, dev))
                timed("save pinned", lambda: src.save_state(out=pin))
                timed("save pageable", lambda: src.save_state(out=page))
                timed("copy h2d", lambda: copy(dev, pinned))
                restore(pin)
                restore(page)
            assert np.array_equal(pin, page) and np.array_equal(dst.download(0), src.download(0))


def child_create(lib_path):
    from rene_amd import abi, scenes
    try:
        import torch  # noqa: F401  (the same HIP runtime as the other measurements)
    except Exception:
        pass
    L = C.CDLL(lib_path)
    L.rene_create.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Opts), C.POINTER(C.c_void_p)]
    L.rene_destroy.argtypes = [C.c_void_p]
    L.rene_destroy.restype = None
    packed = scenes.dragon_class().to_desc()
    o = abi.Opts()
    o.struct_size, o.seed, o.shard_count = C.sizeof(abi.Opts), abi.DEFAULT_SEED, 1
    for rep in range(6):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = L.rene_create(packed.byref(), C.byref(o), C.byref(h))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        L.rene_destroy(h)
        if rep:
            print(f"[cost] create {ms:.4f}", file=sys.stderr, flush=True)


def stats(v):
    v = sorted(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "n": len(v)}


def run_child(*args, debug=False):
    env = dict(os.environ)
    env.pop("RENE_DEBUG", None)
    if debug:
        env["RENE_DEBUG"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"child {args} failed")
    return p.stderr


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child-state"]:
        return child_state()
    if args[:1] == ["--child-create"]:
        return child_create(args[1])
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "state_cost.json")
    log = run_child("--child-state", debug=False) + run_child("--child-state", debug=True)
    result = {"what": __doc__.split("\n\n")[0], "frames": FRAMES, "repetitions": REPS, "sizes": []}
    section, warm, sections, debug_log = None, True, {}, False
    kernel_of = {"rene_save_state": "save", "rene_restore_state": "restore"}
    pending_kernel = {}
    for line in log.splitlines():
        m = re.match(r"\[cost\] (warm-up|round) (\d+) (\d+) (\d+)", line)
        if m:
            warm = m.group(1) == "warm-up"
            w, h, n = int(m.group(2)), int(m.group(3)), int(m.group(4))
            if w not in sections:
                sections[w] = {"width": w, "height": h, "bytes": n, "raw": {}}
                result["sizes"].append(sections[w])
            section = sections[w]
            continue
        m = re.match(r"\[rene\] (rene_save_state|rene_restore_state) .*, (pinned memory|through the stagings), ms: kernels (\S+), pipeline (\S+)", line)
        if m:  # the library's line comes before the wall time of the call it belongs to
            pending_kernel = {"op": kernel_of[m.group(1)], "kernels": float(m.group(3)), "pipeline": float(m.group(4))}
            debug_log = True  # (the second child's log from here on)
            continue
        m = re.match(r"\[cost\] (copy d2h|copy h2d|save pinned|save pageable|restore pinned|restore pageable) (\S+)", line)
        if m and section is not None and not warm:
            if not debug_log and not pending_kernel:
                section["raw"].setdefault(m.group(1), []).append(float(m.group(2)))
            elif m.group(1).startswith(("save", "restore")):
                section["raw"].setdefault(m.group(1) + ", wall under the events", []).append(float(m.group(2)))
            if pending_kernel and m.group(1).startswith(pending_kernel["op"]):
                section["raw"].setdefault(m.group(1) + ", kernels (HIP events, summed over the chunks)", []).append(pending_kernel["kernels"])
                section["raw"].setdefault(m.group(1) + ", pipeline inside the call, under the events", []).append(pending_kernel["pipeline"])
            pending_kernel = {}
    for section in result["sizes"]:
        raw = section.pop("raw")
        section["ms"] = {k: stats(v) for k, v in raw.items()}
        gb = section["bytes"] / 1e9
        section["GB_per_s_at_the_median"] = {k: round(gb / (v["median_ms"] / 1e3), 2) for k, v in section["ms"].items() if "," not in k}
        for op, yard in (("save pinned", "copy d2h"), ("save pageable", "copy d2h"), ("restore pinned", "copy h2d"), ("restore pageable", "copy h2d")):
            if op in section["ms"] and yard in section["ms"]:
                y = section["ms"][yard]
                section.setdefault("above_the_bare_copy_ms", {})[op] = {"difference_of_medians": round(section["ms"][op]["median_ms"] - y["median_ms"], 4),
                                                                        "the_copy's_own_range": round(y["max_ms"] - y["min_ms"], 4)}
    if parent:
        this = os.path.join(ROOT, "rene_amd", "csrc", "librene_hip.so")
        runs = {"this build": [], "parent": []}
        for _ in range(3):  # alternating
            for name, path in (("parent", parent), ("this build", this)):
                runs[name].append([float(x) for x in re.findall(r"\[cost\] create (\S+)", run_child("--child-create", path))])
        result["rene_create on dragon_class(), ms"] = {
            name: {"per run (median of five)": [round(float(np.median(r)), 3) for r in rs], **stats([x for r in rs for x in r])} for name, rs in runs.items()}
        a, b = result["rene_create on dragon_class(), ms"]["this build"], result["rene_create on dragon_class(), ms"]["parent"]
        result["rene_create on dragon_class(), ms"]["difference of medians"] = round(a["median_ms"] - b["median_ms"], 3)
        result["rene_create on dragon_class(), ms"]["parent's spread (max - min)"] = round(b["max_ms"] - b["min_ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

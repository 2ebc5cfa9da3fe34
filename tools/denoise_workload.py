"""tools/denoise_workload.py W H REPS [ab]: render cornell_box(W, H) at 8 spp, then REPS denoise calls (host clock around each, which ends
in a wait); `ab`: alternate RENE_DENOISE_STAGE_MAX over 4, 0, 2 (REPS rounds).  RENE_DEBUG=1 makes the library print the per-kernel events."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rene_amd import api, scenes

w, h, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
ab = len(sys.argv) > 4 and sys.argv[4] == "ab"
with api.Renderer(scenes.cornell_box(w, h)) as r:
    t = time.perf_counter()
    r.render(0, 8)
    r.sync()
    print(f"render {w}x{h} 8 spp: {(time.perf_counter() - t) * 1e3:.2f} ms host, kernel {r.stats().kernel_ms:.2f} ms", flush=True)
    r.denoise()  # warm-up: allocation, code objects
    for k in range(reps):
        for sm in ((4, 0, 2) if ab else (None,)):
            if sm is not None:
                os.environ["RENE_DENOISE_STAGE_MAX"] = str(sm)
            sys.stderr.flush()
            t = time.perf_counter()
            r.denoise()
            print(f"denoise {w}x{h} stage_max={sm}: {(time.perf_counter() - t) * 1e3:.3f} ms host", flush=True)

"""Records tests/golden/frame_stream_layers.npz: the three layers of Cornell and of Cornell + a distant light, 48 x 40 pixels (ragged 32 x 32
tiles), frames 0 .. 15, with the default flags and with RENE_FLAG_NO_AOV.  Recorded once with the library of the commit BEFORE the frame-wide
sample stream moved into a per-launch table (every lane then drew it itself), so that tests/test_gpu_frame_stream.py holds the table to the
bits of the per-lane code.  Needs a GPU:  python tests/golden/make_frame_stream_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rene_amd import abi, api, scenes  # noqa: E402

W, H, FRAMES, SPLIT = 48, 40, 16, 9
SUN = ((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))  # the distant light of sample_scenes/dragon/scene.pbrt:44


def cornell():
    return scenes.cornell_box(W, H)


def cornell_sun():
    s = scenes.cornell_box(W, H)
    s.add_light_distant(*SUN)
    return s


SCENES = {"cornell": cornell, "cornell_sun": cornell_sun}
FLAGS = {"aov": 0, "noaov": abi.FLAG_NO_AOV}


def layers(r):
    return np.stack([r.download(k) for k in range(3)])


def main(out):
    rec = {}
    for sname, make in SCENES.items():
        for fname, flags in FLAGS.items():
            with api.Renderer(make(), flags=flags) as r:
                r.render(0, FRAMES)
                one = layers(r)
                r.reset()
                r.render(0, SPLIT)
                r.render(SPLIT, FRAMES - SPLIT)
                two = layers(r)
            assert np.array_equal(one, two), (sname, fname)
            assert np.isfinite(one).all() and one[0].max() > 0
            rec[f"{sname}_{fname}"] = one
            print(sname, fname, "radiance sum", float(one[0].astype(np.float64).sum()))
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "frame_stream_layers.npz"))

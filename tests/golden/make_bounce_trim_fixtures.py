"""Records the fixtures of tests/test_gpu_bounce_trims.py: the layers and counters of tests/bounce_trim_cases.py's renders, as the library named
by RENE_HIP_LIB (default: this tree's) computes them on the GPU it runs on.

    RENE_HIP_LIB=librene_hip_parent.so python3 tests/golden/make_bounce_trim_fixtures.py [DIR]

The committed files were recorded this way from the build of the commit before RENE_BOUNCE_TRIMS existed (its library copied into csrc/ under
that name); DIR defaults to tests/golden/bounce_trims."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bounce_trim_cases as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else cases.DIR
    os.makedirs(out, exist_ok=True)
    counters = {}
    for name in cases.CASES:
        layers, counters[name] = cases.render_case(name)
        for k in range(3):
            np.save(cases.layer_path(name, k, out), layers[k])
        print(name, layers.shape, counters[name])
    with open(os.path.join(out, "counters.json"), "w") as f:
        json.dump(counters, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

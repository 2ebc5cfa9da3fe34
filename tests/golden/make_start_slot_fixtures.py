"""Records the fixtures of tests/test_gpu_start_slot.py: the layers and counters of tests/start_slot_cases.py's renders, as the library named
by RENE_HIP_LIB (default: this tree's) computes them on the GPU it runs on.

    RENE_HIP_LIB=librene_hip_parent.so python3 tests/golden/make_start_slot_fixtures.py [DIR]

The committed files were recorded this way from the build of the commit before RENE_START_SLOT existed (its library copied into csrc/ under
that name); DIR defaults to tests/golden/start_slot."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import start_slot_cases as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else cases.DIR
    os.makedirs(out, exist_ok=True)
    counters = {}
    for name in cases.CASES:
        layers, counters[name] = cases.render_case(name)
        np.savez_compressed(cases.layers_path(name, out), layers=layers)
        print(name, layers.shape, counters[name])
    with open(os.path.join(out, "counters.json"), "w") as f:
        json.dump(counters, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

"""The two forms of the shading frame (csrc/device_math.h: onb_from_w with its divergent branch, onb_from_w_select without it) against each
other on the device the tests run on (csrc/selftest/onb_probe.hip), under the kernels' own flags: a few thousand random unit normals and the
crafted ones -- |x| == |y|, (0, 0, +-1), the axis normals, +-0 and denormal components, NaN and inf lanes -- with every lane live and with an
irregular half of them dead: u and v bit for bit.  The same binary checks what the static Matte BSDF of the small-scene kernels rests on
(csrc/device_code.inc, TRIM_UNIT_LEN): v_rcp_f32(1.0f) is exactly 1.0f, and a pdf p gives what p * rcp(1) gives through 0.5 * p + q and p < 1e-5,
denormal p included."""
import os
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "rene_amd", "csrc", "selftest", "onb_probe")
N_NORMALS, N_P, N_Q = 4096, 64, 11


@pytest.mark.gpu
def test_both_frames_and_the_unit_division_give_the_same_bits():
    assert os.path.exists(BIN), "build it: make -C rene_amd/csrc"
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr)
    lines = {}
    for line in p.stdout.splitlines():
        if line.split()[0] in ("frame", "rcp1", "pdf"):
            lines.setdefault(line.split()[0], []).append(line.split()[1:])
    assert p.returncode == 0 and len(lines.get("frame", [])) == 2 and len(lines.get("rcp1", [])) == 1 and len(lines.get("pdf", [])) == 1, (p.returncode, p.stdout, p.stderr)
    (all_n, all_bad), (half_n, half_bad) = [(int(a), int(b)) for a, b in lines["frame"]]
    assert all_bad == 0 and half_bad == 0, p.stdout  # 0 mismatched bits in u and v
    assert all_n == N_NORMALS * 6  # every normal, u and v
    assert 0.4 * all_n < half_n < 0.6 * all_n  # an irregular half of the lanes had no normal
    assert lines["rcp1"][0] == ["3f800000"]
    pdf_n, pdf_bad = (int(x) for x in lines["pdf"][0])
    assert pdf_bad == 0 and pdf_n == N_P * N_Q * 2, p.stdout

"""CPU: the render-kernel selection (rene_amd/csrc/kernel_select.h) against kernel_matrix.expected_kernel, the independently written restatement
that the GPU matrix checks against the launch log -- over every input of the selection, which the 24 scenes of that matrix cannot reach:
all 4096 values of the twelve feature bits x the context flags {0, C, N, C|N, R, C|R, N|R} x a main structure of 512 and of 513 nodes x instance
and light tables at the edge of the 40 KB rule x no instance and one x RENE_NO_LDS_TABLES unset and set (458 752 cases, one run of
selftest/kernel_select_dump).

The edge of the 40 KB rule: a 16-entry stack is 16 KB, so the tables have 24 576 bytes -- one Inst (96 bytes) and 765 Lights (32 bytes), or 768
Lights, fit by exactly 0 bytes.  The stack is a multiple of 1 KB and both records are multiples of 32 bytes, so no scene misses the rule by 16
bytes: the closest miss, one Light more, is by 32."""
import os
import re
import subprocess
from types import SimpleNamespace

import kernel_matrix as km
from rene_amd import abi

DUMP = os.path.join(km.CSRC, "selftest", "kernel_select_dump")
_C, _N, _R = abi.FLAG_COUNTERS, abi.FLAG_NO_AOV, abi.FLAG_NO_RESTART
FLAGS = (0, _C, _N, _C | _N, _R, _C | _R, _N | _R)
STACK = 16          # kernel_matrix.stack_entries of a tree at most 16 deep
SMALL_BYTES = 4096  # the LDS image of a FEAT_SMALL scene: what its item-loop kernel has in LDS, whatever the other inputs


def _cases():
    room = km.LDS_TABLES_MAX - STACK * km.BLOCK * 4
    for features in range(4096):
        for flags in FLAGS:
            for n_nodes in (km.RESTART_MIN_NODES, km.RESTART_MIN_NODES + 1):
                for n_insts in (0, 1):
                    fit = (room - n_insts * km.INST_BYTES) // km.LIGHT_BYTES
                    assert STACK * km.BLOCK * 4 + n_insts * km.INST_BYTES + fit * km.LIGHT_BYTES == km.LDS_TABLES_MAX  # fits by exactly 0 bytes
                    for lights in (fit, fit + 1):
                        for no_tables in (False, True):
                            yield features, flags, n_nodes, n_insts, lights, no_tables


def test_selection_is_the_restated_one(hip_lib):
    if not os.path.exists(DUMP):  # (the library was built by hand: `make` builds this with it)
        subprocess.check_call(["make", "-C", km.CSRC, "selftest/kernel_select_dump"])
    assert re.search(r"^constexpr int BLOCK = %d;" % km.BLOCK, open(os.path.join(km.CSRC, "device_code.inc")).read(), re.M)
    cases = list(_cases())
    assert len(cases) == 4096 * 7 * 2 * 2 * 2 * 2
    text = "".join(f"{f} {fl} {n} {STACK} {ni} {li} {SMALL_BYTES if f & km.SMALL else 0} {int(nt)}\n" for f, fl, n, ni, li, nt in cases)
    got = subprocess.run([DUMP, str(km.BLOCK)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(cases)
    stack_bytes = STACK * km.BLOCK * 4
    wrong = []
    for case, line in zip(cases, got):
        f, fl, n, ni, li, nt = case
        info = SimpleNamespace(features=f, n_nodes_main=n, n_instances=ni, lights_len=li, depth_main=STACK, depth_emit=1)
        want = km.expected_kernel(info, fl, nt)
        name, *rest = line.split()
        out = dict(r.split("=") for r in rest)
        wf, tables = "render_kernel_wf" in want, want.endswith("Lb1EEEvNS_9SceneViewENS_12RenderParamsE") and "render_kernel_wf" in want
        item = bool(km.kernel_feat(want) & km.SMALL)
        # what the launch sets up follows from the kernel: the family, the LDS in front of the seed tables, the tables' instances, the stack's depth
        lds = (0 if f & km.VOLPATH else SMALL_BYTES) if item else stack_bytes + (ni * km.INST_BYTES + li * km.LIGHT_BYTES if tables else 0)
        setup = {"family": "item" if item else "restart" if wf else "while", "lds": str(lds), "lds_insts": str(ni if tables else 0),
                 "stack_entries": str(int(wf)),
                 # the two Matte item-loop kernels read the frame-stream table (device_code.inc, frame_stream_feat), nothing else does
                 "reads_frame_stream": str(int(want.startswith(("_ZN4rene13render_kernelILj64E", "_ZN4rene13render_kernelILj72E"))))}
        shade = "matte" if not f & (km.ALL & ~km.LIGHTS) else "multi" if f & km.MULTI else "single"
        if name != want or {k: out[k] for k in setup} != setup or out["shade"] != shade:
            wrong.append((case, line, want, setup))
    assert not wrong, f"{len(wrong)} of {len(cases)} selections differ; the first (case, got, expected kernel, expected set-up): {wrong[0]}"
    # every instantiation a build holds is chosen by some case, and nothing else is
    names = km.res_kernel_names()
    if names is not None:
        chosen = {line.split()[0] for line in got}
        built = {n for n in names if "render_kernel" in n}
        assert chosen == built, (sorted(chosen - built), sorted(built - chosen))

"""CPU: the numpy restatement of the geometry pass (tests/gbuffer_reference.py) on crafted samples, the host side of rene_gbuffer -- struct sizes,
defaults, parameter checks, the Python helpers, the command line's refusals -- and two properties of the inputs the GPU tests use: the oracle's own
records reach the `other` path and four filled slots, and its edge samples stay under the cap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gbuffer_reference as gr
from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
ORIGIN = np.float32([1.0, 2.0, 3.0])


def _one(ts, who, **kw):
    return gr.aggregate(gr.crafted(ts, who), ORIGIN, **kw)[0, 0]


def test_sums_run_in_frame_order_in_fp32():
    ts = np.float32([1e8, 1.0, -1.0, 1.0, 3.25])
    r = _one(ts, [7] * 5)
    want = np.float32(0)
    for t in ts[ts >= 0]:
        want = np.float32(want + t)  # (1e8 swallows the 1.0s: the order shows)
    assert r["depth_sum"] == want and r["depth_min"] == np.float32(1.0) and r["hits"] == 4 and r["n"] == 5
    z = np.float32(0)
    for t in ts[ts >= 0]:
        z = np.float32(z + np.float32(ORIGIN[2] + np.float32(t * np.float32(1.0))))
    assert r["position_sum"][2] == z and r["position_sum"][0] == np.float32(4.0)  # x: four times the origin's
    assert list(r["id"]) == [7, gr.NONE, gr.NONE, gr.NONE] and list(r["count"]) == [4, 0, 0, 0] and r["other"] == 0


def test_a_count_tie_is_broken_by_id():
    r = _one([1, 1, 1, 1, 1], [9, 4, 9, 4, 2])
    assert list(r["id"]) == [4, 9, 2, gr.NONE] and list(r["count"]) == [2, 2, 1, 0]


def test_a_fifth_distinct_id_goes_to_other_and_nothing_is_evicted():
    r = _one([1] * 9, [5, 6, 7, 8, 99, 99, 99, 8, 5])
    assert r["other"] == 3 and list(r["id"]) == [5, 8, 6, 7] and list(r["count"]) == [2, 2, 1, 1] and r["hits"] == 9


def test_all_misses_and_an_unowned_pixel():
    r = _one([-1, -1, -1], [0, 0, 0])
    assert r["depth_min"] == np.inf and r["depth_sum"] == 0 and r["hits"] == 0 and r["n"] == 3 and not r["position_sum"].any()
    assert (r["id"] == gr.NONE).all() and not r["count"].any()
    z = gr.aggregate(gr.crafted([1, 2], [3, 3]), ORIGIN, owned=np.zeros((1, 1), bool))
    assert z.tobytes() == bytes(64)  # n = 0: all zero


def test_material_ids_go_through_the_instance_table():
    r = _one([1, 1, 1], [0, 1, 2], ids="material", materials=[5, 5, 3])
    assert list(r["id"][:2]) == [5, 3] and list(r["count"][:2]) == [2, 1]


def test_merge_and_helpers():
    s = np.zeros((3, 2, 4), abi.PRIMARY_HIT_DTYPE)
    s["t"] = np.random.default_rng(1).uniform(0.5, 4.0, s.shape).astype(np.float32)
    s["t"][0, 0, 0] = s["t"][1, 0, 0] = s["t"][2, 0, 0] = -1
    s["d"][..., 2] = 1
    s["instance"] = np.arange(8).reshape(2, 4) % 3
    full = gr.aggregate(s, ORIGIN)
    left = np.zeros((2, 4), bool)
    left[:, :2] = True
    parts = [gr.aggregate(s, ORIGIN, owned=left), gr.aggregate(s, ORIGIN, owned=~left)]
    assert api.gbuffer_merge(parts).tobytes() == full.tobytes() and api.gbuffer_merge(parts[::-1]).tobytes() == full.tobytes()
    with pytest.raises(ValueError):
        api.gbuffer_merge([parts[0], parts[0]])
    depth, cov, pos = api.gbuffer_depth(full), api.gbuffer_coverage(full), api.gbuffer_position(full)
    assert depth[0, 0] == np.inf and cov[0, 0] == 0 and not pos[0, 0].any()
    assert depth[1, 1] == full["depth_sum"][1, 1] / np.float32(3) and cov[1, 1] == 1 and (pos[1, 1] == full["position_sum"][1, 1] / np.float32(3)).all()
    assert api.gbuffer_coverage(parts[0])[0, 3] == 0  # n == 0
    assert api.gbuffer_matte(full, 1)[0, 1] == 1 and api.gbuffer_matte(full, 2)[0, 1] == 0 and api.gbuffer_matte(full, 0)[0, 0] == 0


def test_abi_structs_defaults_and_symbols(hip_lib):
    assert C.sizeof(abi.GbufferPixel) == 64 == np.dtype(abi.GBUFFER_DTYPE).itemsize
    assert C.sizeof(abi.PrimaryHit) == 32 == np.dtype(abi.PRIMARY_HIT_DTYPE).itemsize and C.sizeof(abi.GbufferParams) == 20
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rene_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %u\\n", sizeof(rene_gbuffer_pixel), '
            'sizeof(rene_primary_hit), sizeof(rene_gbuffer_params), offsetof(rene_gbuffer_pixel, position_sum), offsetof(rene_gbuffer_pixel, id), '
            'offsetof(rene_primary_hit, u), RENE_ABI_VERSION);return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])  # (the header is C)
        assert subprocess.check_output([exe]).split() == [b"64", b"32", b"20", b"16", b"32", b"16", b"7"]
    for name in ("rene_gbuffer_params_default", "rene_gbuffer_bytes", "rene_gbuffer", "rene_gbuffer_buffer", "rene_download_gbuffer", "rene_primary_hits"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    p = api.gbuffer_params_default()
    assert (p.struct_size, p.first_frame, p.n_frames, p.id_source, p.flags) == (20, 0, 16, abi.GBUFFER_ID_INSTANCE, 0)
    assert api.gbuffer_bytes(77, 45) == 77 * 45 * 64 and api.gbuffer_bytes(16384, 16384) == 64 << 28 and api.gbuffer_bytes(0, 9) == 0
    for m in ("gbuffer", "gbuffer_into", "gbuffer_buffer", "primary_hits"):
        assert callable(getattr(api.Renderer, m))


def test_parameters_are_checked_and_nothing_runs_without_a_gpu(hip_lib):
    L = hip_lib
    err = lambda: L.rene_last_error().decode()
    buf = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    for field, value, word in (("struct_size", 16, "struct_size"), ("n_frames", 0, "n_frames"), ("n_frames", 65537, "n_frames"),
                               ("id_source", 3, "id_source"), ("flags", 1, "flags")):
        p = api.gbuffer_params_default()
        setattr(p, field, value)
        assert L.rene_gbuffer(None, C.byref(p), None, 0) == -1 and word in err(), field
    # good parameters: what is missing is the context -- there is none without a GPU, and no CPU fallback
    assert L.rene_gbuffer(None, C.byref(api.gbuffer_params_default()), None, 0) == -1 and "NULL context" in err()
    assert L.rene_gbuffer(None, None, None, 0) == -1 and "NULL context" in err()
    for n in (0, 65537):
        assert L.rene_primary_hits(None, 0, n, buf, 2) == -1 and "n_frames" in err()
    assert L.rene_primary_hits(None, 0, 4, buf, 2) == -1 and "NULL" in err()
    p, n = C.c_void_p(), C.c_size_t()
    assert L.rene_gbuffer_buffer(None, C.byref(p), C.byref(n)) == -1 and L.rene_download_gbuffer(None, buf, 64) == -1
    with pytest.raises(ValueError):
        api._gbuffer_params(0, 4, "object")
    from conftest import has_gpu
    if not has_gpu():
        with pytest.raises(api.ReneError) as e:
            api.Renderer(scenes.cornell_box(16, 16)).gbuffer()
        assert e.value.code == -3  # RENE_ERR_DEVICE


def test_the_command_line_refuses_before_it_loads_anything(hip_lib):
    def run(*args):
        return subprocess.run([CLI, "no-such.pbrt", *args], capture_output=True, text=True)
    r = run("--gbuffer", "g", "--gpus", "2")
    assert r.returncode == 2 and "rene_gbuffer" in r.stderr and "api.gbuffer_merge" in r.stderr
    r = run("--gbuffer", "g", "--gbuffer-id", "object")
    assert r.returncode == 2 and "--gbuffer-id" in r.stderr
    assert run("--gbuffer-id", "objects").returncode == 2 and run("--gbuffer").returncode == 2  # (a missing value)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gbuffer PREFIX" in r.stderr and "--checkpoint FILE" in r.stderr and "--features PREFIX" in r.stderr


def test_the_reference_reaches_other_and_four_slots(oracle_mod):
    """matte-deep+emitter, ids="primitive", frames 3 .. 18: the displaced sphere's silhouette and its small triangles give pixels whose 16 samples
    see five primitives and more.  The GPU test of the `other` path uses exactly these inputs."""
    ref = gr.reference(gr.OTHER_SCENE)
    assert ref["samples"].shape[0] == gr.OTHER_FRAMES == 16
    rec = gr.aggregate(ref["samples"], ref["origin"], "primitive")
    filled = (rec["count"] > 0).sum(-1)
    print("pixels with other > 0:", int((rec["other"] > 0).sum()), "with exactly four slots and no other:", int(((filled == 4) & (rec["other"] == 0)).sum()))
    assert (rec["other"] > 0).any() and ((filled == 4) & (rec["other"] == 0)).any()
    assert (rec["hits"] == rec["count"].sum(-1) + rec["other"]).all()


@pytest.mark.parametrize("name", gr.SCENES)
def test_edge_samples_stay_under_the_cap(name, oracle_mod):
    ref = gr.reference(name)
    share = ref["edge"].mean()
    print(name, "edge samples:", int(ref["edge"].sum()), "of", ref["edge"].size, f"= {share:.4%}")
    assert share <= gr.EDGE_CAP
    hit = ref["samples"]["t"] >= 0
    assert 0.3 < hit.mean() <= 1.0  # the film sees the room

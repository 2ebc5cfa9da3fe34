"""CPU: the host side of the light-group pass (rene_lights, include/rene_hip.h) -- the header as C99, struct sizes and offsets against the ctypes
mirrors, defaults, the ABI version, every refusal that needs no GPU, and the command line's refusals and --help.  (rene_lights_default_groups
takes a context, which needs a device: its overflow into group 7 is held in tests/test_gpu_lights.py; the restatement the tests group by is
held here.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lights_scenes
from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
SYMBOLS = ("rene_lights_params_default", "rene_lights_bytes", "rene_lights_default_groups", "rene_lights", "rene_lights_buffer", "rene_download_lights",
           "rene_lights_samples")


def test_abi_structs_defaults_and_symbols(hip_lib):
    assert C.sizeof(abi.LightsPixel) == 144 == np.dtype(abi.LIGHTS_DTYPE).itemsize
    assert C.sizeof(abi.LightsSample) == 144 == np.dtype(abi.LIGHTS_SAMPLE_DTYPE).itemsize
    assert C.sizeof(abi.LightsParams) == 48 and C.sizeof(abi.LightsGroup) == 16 == np.dtype(abi.LIGHTS_GROUP_DTYPE).itemsize
    fields = ("sizeof(rene_lights_params)", "sizeof(rene_lights_pixel)", "sizeof(rene_lights_sample)", "sizeof(rene_lights_group)",
              "offsetof(rene_lights_params, flags)", "offsetof(rene_lights_params, n_instances)", "offsetof(rene_lights_params, n_distant)",
              "offsetof(rene_lights_params, instance_group)", "offsetof(rene_lights_params, distant_group)", "offsetof(rene_lights_params, background_group)",
              "offsetof(rene_lights_group, adds)", "offsetof(rene_lights_pixel, group[7])", "offsetof(rene_lights_pixel, n)", "offsetof(rene_lights_pixel, lit)",
              "offsetof(rene_lights_pixel, reserved)", "offsetof(rene_lights_sample, n)", "offsetof(rene_lights_sample, lit)",
              "offsetof(rene_lights_sample, length)", "offsetof(rene_lights_sample, end)", "(size_t)RENE_LIGHTS_MAX_FRAMES", "(size_t)RENE_LIGHTS_GROUPS",
              "(size_t)RENE_ABI_VERSION")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rene_hip.h"\nint main(void){size_t v[] = {' + ", ".join(fields) +
            '};for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])  # (the header is C)
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [48, 144, 144, 16, 12, 16, 20, 24, 32, 40, 12, 112, 128, 132, 136, 128, 132, 136, 140, 65536, 8, 7]
    A, P, S = abi.LightsParams, abi.LightsPixel, abi.LightsSample
    assert (A.flags.offset, A.n_instances.offset, A.n_distant.offset, A.instance_group.offset, A.distant_group.offset, A.background_group.offset) == (12, 16, 20, 24, 32, 40)
    assert (P.group.offset, P.n.offset, P.lit.offset, P.reserved.offset) == (0, 128, 132, 136)
    assert (S.group.offset, S.n.offset, S.lit.offset, S.length.offset, S.end.offset) == (0, 128, 132, 136, 140)
    assert (abi.LightsGroup.sum.offset, abi.LightsGroup.adds.offset) == (0, 12)
    for dtype, struct in ((abi.LIGHTS_DTYPE, P), (abi.LIGHTS_SAMPLE_DTYPE, S), (abi.LIGHTS_GROUP_DTYPE, abi.LightsGroup)):
        d = np.dtype(dtype)
        assert {k: d.fields[k][1] for k in d.names} == {k: getattr(struct, k).offset for k, _ in struct._fields_}
    assert np.dtype(abi.LIGHTS_DTYPE).fields["group"][0].shape == (8,)
    assert (abi.LIGHTS_MAX_FRAMES, abi.LIGHTS_GROUPS) == (65536, 8)
    assert abi.ABI_VERSION == 7 == hip_lib.rene_abi_version()  # added symbols: no version change
    for name in SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    p = api.lights_params_default()
    assert (p.struct_size, p.first_frame, p.n_frames, p.flags, p.n_instances, p.n_distant, p.instance_group, p.distant_group, p.background_group) == \
        (48, 0, 16, 0, 0, 0, None, None, 0)
    assert api.lights_bytes(72, 40) == 72 * 40 * 144 and api.lights_bytes(16384, 16384) == 144 << 28 and api.lights_bytes(0, 9) == 0
    for m in ("lights", "lights_into", "lights_buffer", "lights_samples", "light_groups"):
        assert callable(getattr(api.Renderer, m))
    for f in ("lights_sum", "lights_group_sum", "lights_group_mean", "lights_mix", "lights_merge"):
        assert callable(getattr(api, f))
    hip_lib.rene_lights_params_default(None)  # (a NULL destination: nothing happens)


BAD = (("struct_size", 44, "struct_size"), ("struct_size", 0, "struct_size"), ("n_frames", 0, "n_frames"), ("n_frames", 65537, "n_frames"),
       ("flags", 1, "flags"), ("flags", 1 << 31, "flags"))


def _with_tables(inst, dist, bg=0):
    p = api.lights_params_default()
    inst, dist = np.asarray(inst, np.uint8), np.asarray(dist, np.uint8)
    p.n_instances, p.n_distant, p.background_group = inst.size, dist.size, bg
    p.instance_group, p.distant_group = (inst.ctypes.data if inst.size else None), (dist.ctypes.data if dist.size else None)
    return p, (inst, dist)


def test_parameters_are_checked_and_nothing_runs_without_a_gpu(hip_lib):
    L = hip_lib
    err = lambda: L.rene_last_error().decode()
    buf = np.zeros(512, np.uint8).ctypes.data_as(C.c_void_p)
    for field, value, word in BAD:
        p = api.lights_params_default()
        setattr(p, field, value)
        assert L.rene_lights(None, C.byref(p), None, 0) == -1 and word in err() and "rene_lights" in err(), (field, value)
        assert L.rene_lights_samples(None, C.byref(p), buf, 2) == -1 and word in err() and "rene_lights" in err(), (field, value)
    # a NULL table with a count above 0
    for field in ("n_instances", "n_distant"):
        p = api.lights_params_default()
        setattr(p, field, 3)
        assert L.rene_lights(None, C.byref(p), None, 0) == -1 and "NULL table" in err(), field
        assert L.rene_lights_samples(None, C.byref(p), buf, 2) == -1 and "NULL table" in err(), field
    # an entry of 8 or more, wherever it stands, and a background group of 8
    for inst, dist, bg, word in (([0, 1, 8], [1], 0, "instance_group[2]"), ([255, 1], [], 0, "instance_group[0]"), ([0, 7], [2, 9], 0, "distant_group[1]"),
                                 ([0, 7], [7], 8, "background_group"), ([0], [], 255, "background_group")):
        p, keep = _with_tables(inst, dist, bg)
        assert L.rene_lights(None, C.byref(p), None, 0) == -1 and word in err() and "below 8" in err(), word
        assert L.rene_lights_samples(None, C.byref(p), buf, 2) == -1 and word in err(), word
    # the ends of the ranges are inside them: what is missing then is the context
    for field, value in (("n_frames", 1), ("n_frames", 65536)):
        p = api.lights_params_default()
        setattr(p, field, value)
        assert L.rene_lights(None, C.byref(p), None, 0) == -1 and "rene_lights: NULL context" in err(), (field, value)
    p, keep = _with_tables([0, 7, 3], [7, 0], 7)
    assert L.rene_lights(None, C.byref(p), None, 0) == -1 and "rene_lights: NULL context" in err()
    assert L.rene_lights(None, None, None, 0) == -1 and err() == "rene_lights: NULL context"
    assert L.rene_lights_samples(None, None, buf, 2) == -1 and "rene_lights_samples: NULL" in err()
    ptr, n = C.c_void_p(), C.c_size_t()
    assert L.rene_lights_buffer(None, C.byref(ptr), C.byref(n)) == -1 and "rene_lights_buffer" in err() and "NULL" in err()
    assert L.rene_download_lights(None, buf, 288) == -1 and "rene_download_lights" in err() and "NULL" in err()
    bg, used = C.c_uint8(), C.c_uint32()
    assert L.rene_lights_default_groups(None, None, 0, None, 0, C.byref(bg), C.byref(used)) == -1 and "rene_lights_default_groups: NULL context" in err()
    from conftest import has_gpu
    if not has_gpu():
        with pytest.raises(api.ReneError) as e:
            api.Renderer(scenes.cornell_box(16, 16)).lights()
        assert e.value.code == -3  # RENE_ERR_DEVICE


def test_the_restated_grouping_of_the_test_scenes():
    """Group 0 the background, the distant lights, then the emitting instances in instance order; past seven sources the rest share group 7."""
    s = lights_scenes.cornell()
    (inst, dist, bg), used = lights_scenes.default_groups(s)
    assert (bg, used, dist.tolist()) == (0, 4, [1]) and inst.tolist() == [0] * 7 + [2, 3]
    (inst, dist, bg), used = lights_scenes.default_groups(lights_scenes.zoo())
    assert (bg, used, dist.tolist()) == (0, 4, [1]) and sorted(inst[inst != 0].tolist()) == [2, 3]
    many = lights_scenes.many_sources()
    (inst, dist, bg), used = lights_scenes.default_groups(many)
    assert used == 8 and dist.tolist() == [1, 2, 3] and inst[lights_scenes.emitting(many)].tolist() == [4, 5, 6, 7, 7, 7]
    black = lights_scenes.only(lights_scenes.cornell, 2)
    assert [tuple(a.v0[:3]) for a in black.area_lights[1:]] == [(17.0, 12.0, 4.0), (0.0, 0.0, 0.0)] and tuple(black.lights[0].v1[:3]) == (0.0, 0.0, 0.0)
    assert all(a.type == abi.AREA_LIGHT_DIFFUSE for a in black.area_lights[1:])  # black, and still in its table
    twice = lights_scenes.scaled(lights_scenes.cornell, 3, 2)
    assert [tuple(a.v0[:3]) for a in twice.area_lights[1:]] == [(17.0, 12.0, 4.0), (4.0, 12.0, 18.0)] and tuple(twice.lights[0].v1[:3]) == (3.0, 3.0, 3.0)


def test_the_command_line_refuses_before_it_loads_anything(hip_lib):
    def run(*args):
        return subprocess.run([CLI, "no-such.pbrt", *args], capture_output=True, text=True)
    r = run("--lights", "l", "--gpus", "2")
    assert r.returncode == 2 and "rene_lights" in r.stderr and "api.lights_merge" in r.stderr
    r = run("--lights", "l", "--lights-frames", "65537")
    assert r.returncode == 2 and "--lights-frames" in r.stderr
    for bad in ("1,2,3,4,5,6,7,8,9", "1,,2", "x", "1,2,"):
        r = run("--lights", "l", "--lights-mix", bad)
        assert r.returncode == 2 and "--lights-mix" in r.stderr, bad
    r = run("--lights-mix", "1,2")
    assert r.returncode == 2 and "--lights-mix needs --lights" in r.stderr
    assert run("--lights").returncode == 2 and run("--lights", "l", "--lights-frames").returncode == 2  # (a missing value)
    assert run("--lights", "l", "--lights-mix").returncode == 2
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("--lights PREFIX", "--lights-frames N", "--lights-mix W0,W1,...", "PREFIX.group<k>.pfm", "PREFIX.groups.txt", "PREFIX.mix.pfm", "--bounces PREFIX"):
        assert word in r.stderr, word

"""CPU: the host logic of bench.py that needs no GPU -- its configurations, the roofline arithmetic against the committed
per-ray records, and the child-process harness of the additional configurations (a child that fails or stalls must become an
error entry, not a missing headline line)."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_configurations_and_records():
    cfgs = bench.configurations()
    assert list(cfgs)[0] == "cornell" and set(cfgs) == {"cornell", "veach-mis", "dragon-class", "dragon-partial", "material-zoo", "teapot-class"}
    for name, (label, make, spp, fpl) in cfgs.items():
        assert spp == fpl and callable(make) and str(spp) in label  # one launch per job
        rec = bench.pmc_per_ray(name)
        if name in ("dragon-partial", "material-zoo"):  # timed only: no PMC passes of their own
            continue
        assert rec and rec["valu_wave_insts_per_ray"] > 0 and os.path.exists(os.path.join(ROOT, rec["source"])), name


def test_pmc_staleness_is_reported():
    """the per-ray instruction / byte counts come from committed profiles; bench.py says when the kernel sources
    have changed since (kernel_source_hash stamped by tools/summarize_profiles.py)."""
    h = bench.kernel_source_hash()
    assert len(h) == 16 and h == bench.kernel_source_hash()
    rl = bench.rooflines("cornell", 1.0e11, 256, 500.0)
    rec = bench.pmc_per_ray("cornell")
    assert rl["valu"]["pmc_stale"] == (rec.get("kernel_source_hash") != h)
    assert 0.0 < rl["valu"]["useful_lane_frac"] <= rl["valu"]["frac"]


def test_roofline_fractions_are_fractions():
    for name in bench.configurations():
        if name in ("dragon-partial", "material-zoo"):
            continue
        rl = bench.rooflines(name, 1.0e10 if name != "cornell" else 1.2e11, 256, 500.0)
        assert 0.0 < rl["valu"]["frac"] <= 1.0 and rl["valu"]["peak"] == pytest.approx(78.6432)
        assert 0.0 <= rl["hbm"]["frac"] <= 1.0 and rl["hbm"]["peak"] == 8000.0


def test_a_failing_or_stalling_configuration_becomes_an_error_entry(monkeypatch, tmp_path):
    """configs_in_children runs `bench.py --config-child NAME` per configuration; here the 'bench.py' it starts is a stand-in
    that succeeds for one name, fails for another and sleeps past the timeout for the third."""
    fake = tmp_path / "fake_bench.py"
    fake.write_text(
        "import json, sys, time\n"
        "name = sys.argv[sys.argv.index('--config-child') + 1]\n"
        "if name == 'veach-mis': print(json.dumps({'config': {'value': 1.0}}))\n"
        "elif name == 'dragon-class': sys.stderr.write('boom'); sys.exit(3)\n"
        "else: time.sleep(30)\n")
    monkeypatch.setattr(bench, "__file__", str(fake))
    out = bench.configs_in_children("cornell", timeout_s=2.0)
    assert out["veach-mis"] == {"value": 1.0}
    assert "exit code 3" in out["dragon-class"]["error"] and "boom" in out["dragon-class"]["stderr_tail"]
    assert "did not finish" in out["teapot-class"]["error"] and "did not finish" in out["dragon-partial"]["error"] and "did not finish" in out["material-zoo"]["error"]
    json.dumps(out)


def test_the_committed_bench_line_carries_every_configuration():
    """bench.py's `configs` (the latest committed line under profiles/): every BASELINE configuration beside the headline one, each rendered by
    the library's default path -- since round 4 eight frame chains per pixel on every kernel (`frame_chains`); round 3's lines timed the BVH
    configurations twice (strict frame order and two opt-in chains)."""
    import glob
    path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench.json")))[-1]
    d = json.loads(open(path).read().strip().splitlines()[-1])
    assert d["roofline"]["pmc_stale"] is False, path
    for name in ("veach-mis", "dragon-class", "teapot-class", "dragon-partial", "material-zoo"):
        c = d["configs"][name]
        assert c["value"] > 0 and c["rays"] > 0, name
        if "frame_chains" in c:
            assert c["frame_chains"] == 8 and "strict_order" not in c, name
        else:  # a round-3 line
            assert c["frame_groups"] in (1, 2), name


def test_the_watchdog_turns_a_hung_phase_into_an_error_record_and_a_non_zero_exit():
    """`bench.py --gpus N` must not hang the driver's one scaling run.  A phase that overruns (here: a sleep standing in for
    a rendezvous that never completes) makes rank 0 print ONE JSON error record -- same leading keys as the bench line, value null -- and the
    process leaves with exit code 3, from the watchdog's thread (the main thread never returns); a phase that ends in time leaves no trace."""
    import subprocess
    code = ("import sys, time; sys.path.insert(0, %r)\n"
            "import bench\n"
            "w = bench.Watchdog(0, 2, 2)\n"
            "w.arm('quick phase', 5.0); w.disarm()\n"
            "w.arm('rendezvous that never completes', 0.5)\n"
            "time.sleep(30)\n"
            "print('NOT REACHED')\n" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=25)
    assert p.returncode == 3, (p.returncode, p.stderr[-300:])
    assert "NOT REACHED" not in p.stdout
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["value"] is None and rec["n_gpus"] == 2 and "rendezvous that never completes" in rec["error"] and rec["metric"] == "Mrays/s"
    # a rank other than 0 leaves as loudly, without a record
    p = subprocess.run([sys.executable, "-c", code.replace("Watchdog(0, 2, 2)", "Watchdog(1, 2, 2)")], capture_output=True, text=True, timeout=25)
    assert p.returncode == 3 and p.stdout.strip() == "" and "giving up" in p.stderr


class _StubRenderer:
    """What dump_outputs uses of api.Renderer: the image size and rene_download's [H][W][3] f32 layers."""

    def __init__(self, w, h):
        self.xres, self.yres = w, h

    def download(self, layer, channels=3):
        import numpy as np
        assert channels == 3
        return (np.arange(self.yres * self.xres * 3, dtype=np.float32).reshape(self.yres, self.xres, 3) + 1e6 * layer)


def test_dump_outputs_writes_every_layer_whole_under_the_cap(tmp_path):
    import numpy as np
    r = _StubRenderer(32, 16)
    bench.dump_outputs(r, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["albedo.npy", "normal.npy", "radiance.npy"]
    for layer, name in enumerate(bench.DUMP_LAYERS):
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, r.download(layer))


def test_dump_outputs_samples_a_larger_image_the_same_way_every_time(tmp_path, monkeypatch):
    """Above DUMP_BYTES_MAX: every layer keeps the same seeded pixels, pixel_index.npy holds their row-major indices
    exactly, the files stay under the cap, and a second run writes the same bytes."""
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 64 << 10)  # 64 KB: a 100 x 80 image (3 x 96 KB) must be sampled
    r = _StubRenderer(100, 80)
    for d in ("a", "b"):
        bench.dump_outputs(r, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["albedo.npy", "normal.npy", "pixel_index.npy", "radiance.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES_MAX
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) > 0 and (np.diff(idx) > 0).all() and idx[-1] < 100 * 80
    assert np.array_equal(idx, np.round(idx))
    for layer, name in enumerate(bench.DUMP_LAYERS):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (len(idx), 3)
        assert np.array_equal(a, r.download(layer).reshape(-1, 3)[idx.astype(np.int64)])

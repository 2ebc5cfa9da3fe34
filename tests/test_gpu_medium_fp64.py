"""-m gpu: the device media code -- medium_tr, medium_sample, medium_phase, medium_sample_p -- and the transmittance walks (tr / tr_emit) per
sample against the fp64 reference of tests/medium_reference.py, whose allowance comes from its own sensitivity, from operation counts and
from the ASSUMED exp / log / sin / cos bounds its module docstring names, never from this kernel's output.  tests/test_medium_reference.py
shows on the CPU that the reference meets closed forms it was not written from, that the oracle passes the same check() on the same inputs,
and that the inputs stay within their set-aside caps.

The media go through rene_medium_eval on one context of the shared scene (33 media: the vacuum; grey with g = 0, +-0.3 .. +-0.999 and three
values of either sign around the 1e-3 switch; chromatic, one empty channel, sigma_s = 0, sigma_a = 0, thin, dense and the loader's defaults
at g = 0 and 0.7; dense at -0.99), per medium on 2 048 uniform rows and the named edge rows: every quantity within the allowance wherever the
reference's own rule does not set the sample aside; a flush sample within the allowance of either admissible answer; and on every sample the
class checks (finite, tr in [0, 1], phase >= 0, 0 <= weight <= 3, |p| = 1, the stream's next word).  The walks go through rene_transmittance on
four scenes, on the item loop and on the BVH: tr within the allowance and the query count exact on every ray not set aside.

Largest error / allowance observed on an MI355X (a record, not a threshold; the oracle's own on the same inputs in brackets), uniform / edge:
  tr        0.98 / 0.70 (0.30 / 0.13) -- the device's are denormals flushed to 0 against the 2^-126 every result carries (dense; optical depth 87.7)
  phase     0.33 / 0.20 (0.34 / 0.25)
  position  1.00 / 0.64 (1.00 / 0.64) -- t_max rd of an unsampled row: one rounding against an allowance of one
  weight    0.22 / 0.13 (0.22 / 0.10)
  p         0.40 / 0.51 (0.59 / 0.54)
  walks     slabs 0.005 (0.006), thin 0.001 (0.004), shells 0.031 (0.068), ellipsoid 0.145 (0.116), the same on the item loop and the BVH
Of 41 flush rows (chromatic and one-empty-channel media) the device's weight sits on the flushed answer alone in 7, on the IEEE answer alone in
0, and where the two coincide in 34; the oracle's on the IEEE answer in 7 and on both in 34.  No NaN, inf or weight above 3; no device defect.

Scratch builds of device_code.inc with one line reverted each fail here (tried first on scratch copies of the oracle, on the CPU, through the
same check()):
  1. the density without `sigma_t *` on the sampled side       -- test_the_uniform_set[chromatic g=0.0] (the class check `0 <= weight <= 3` on 510 rows, then the weight's allowance)
  2. `- 2 g cos` in the phase                                   -- test_the_uniform_set[grey g=0.3] (phase)
  3. `g < 1e-3f` without fabsf                                  -- test_the_uniform_set[grey g=-0.3] (p)
  4. exterior / interior swapped in the walk                    -- test_the_walks[slabs-0]
  5. medium_tr without length(rd)                               -- test_the_uniform_set[grey g=0.0] (tr), test_the_walks[slabs-0]
  6. the walk's EMIT return without the facing test             -- test_the_walks[slabs-0] (the averted emitter)
  7. the walk's restart kept, but tmin 0                        -- test_the_walks[thin-0] (the second boundary of a pair is met)
"""
import numpy as np
import pytest

import medium_reference as mr
from rene_amd import abi, api

pytestmark = pytest.mark.gpu

S = mr.shared_scene()


@pytest.fixture(scope="module")
def context():
    with api.Renderer(S.scene) as r:
        yield r


def _held(context, oracle_mod, case, which):
    I = mr.input_set(case, which)
    rows = context.medium_eval(S.index[case], I.rd, I.t_max, I.wo, I.wi, I.seeds)
    result, classes, flush = mr.check(rows, case, which)
    oracle, _, oflush = mr.check(mr.oracle_rows(oracle_mod, case, which), case, which)
    print(f"{case} {which}: error / allowance " + ", ".join(f"{q} {result[q][0]:.2f} ({oracle[q][0]:.2f})" for q in mr.QUANTITIES)
          + f"; flush rows {flush['rows']}: on the IEEE answer {flush['ieee']}, on the flushed {flush['flushed']}, on both {flush['both']}"
          + f" (oracle {oflush['ieee']}, {oflush['flushed']}, {oflush['both']})")
    name = lambda bad: [I.names[i] for i in np.nonzero(bad)[0]] if I.names else np.nonzero(bad)[0][:8]
    for k, bad in classes.items():
        assert not bad.any(), (case, which, k, int(bad.sum()), name(bad), rows[bad][:3])
    for q, (_, bad) in result.items():
        assert not bad.any(), (case, which, q, int(bad.sum()), name(bad), rows[bad][:3])


@pytest.mark.parametrize("case", mr.CASES)
def test_the_uniform_set(case, context, oracle_mod):
    _held(context, oracle_mod, case, "uniform")


@pytest.mark.parametrize("case", mr.CASES)
def test_the_edge_rows(case, context, oracle_mod):
    _held(context, oracle_mod, case, "edge")


@pytest.fixture(scope="module")
def walk_contexts():
    """One context per scene and flag value, made when first asked for."""
    made = {}

    def get(scene, flags):
        if (scene, flags) not in made:
            made[scene, flags] = api.Renderer(mr.walk_scene(scene), flags=flags)
        return made[scene, flags]
    yield get
    for r in made.values():
        r.close()


@pytest.mark.parametrize("scene,start", mr.WALK_CASES, ids=[f"{s}-{m}" for s, m in mr.WALK_CASES])
def test_the_walks(scene, start, walk_contexts, oracle_mod):
    info = api.pack_info(mr.walk_scene(scene))
    assert info.features & (64 | 128) == 64 | 128  # FEAT_SMALL | FEAT_VOLPATH: flags 0 takes the item loop, FLAG_FORCE_BVH clears FEAT_SMALL (the tree)
    ro, rd = mr.walk_rays(scene, start)
    o = oracle_mod.Oracle(mr.walk_scene(scene))
    family = {}
    for flags in (0, abi.FLAG_FORCE_BVH):
        r = walk_contexts(scene, flags)
        out = {}
        for emit in (False, True):
            got = out[emit] = r.transmittance(emit, start, ro, rd)
            worst, bad, count = mr.walk_check(got, scene, start, emit)
            oworst, _, _ = mr.walk_check(o.transmittance(emit, start, ro, rd), scene, start, emit)
            print(f"{scene} from medium {start}, {'bvh' if flags else 'item loop'}, emit {int(emit)}: error / allowance {worst:.3f} ({oworst:.3f})")
            assert not bad.any(), (scene, start, flags, emit, np.nonzero(bad)[0][:8], got[bad][:3])
            assert not count.any(), (scene, start, flags, emit, "query count", np.nonzero(count)[0][:8], got[count][:3])
        # tr and tr_emit on the rays that meet no light: the same queries; a Matte wall ends both at 0, a miss ends tr_emit at 0 (lib.rs:391-394, 445-453)
        ref = mr.walk_reference(scene, start, True)
        keep = ~ref.aside
        blocked, miss = keep & (ref.ended == 1), keep & (ref.ended == 0)
        assert (out[False][blocked, :3] == 0).all() and (out[True][blocked, :3] == 0).all() and (out[True][miss, :3] == 0).all()
        assert (out[False][blocked | miss, 3] == out[True][blocked | miss, 3]).all()
        family[flags] = out
    keep = ~mr.walk_reference(scene, start, False).aside
    assert (family[0][False][keep, 3] == family[abi.FLAG_FORCE_BVH][False][keep, 3]).all()  # both families trace the same queries


def test_the_walk_probe_refuses_what_it_cannot_run(walk_contexts):
    from rene_amd import scenes
    r = walk_contexts("thin", 0)
    ro, rd = mr.walk_rays("thin", 0)
    with pytest.raises(api.ReneError) as e:
        r.transmittance(False, len(mr.walk_description("thin").media), ro[:4], rd[:4])
    assert e.value.code == -1
    assert r.transmittance(True, 0, ro[:0], rd[:0]).shape == (0, 4)
    with api.Renderer(scenes.cornell_box(16, 16)) as path:  # the path integrator: no media on the device
        with pytest.raises(api.ReneError):
            path.transmittance(False, 0, ro[:4], rd[:4])

"""-m gpu: the device BSDF code -- compute_bsdf, lobe_f / lobe_pdf / lobe_sample, the Trowbridge-Reitz functions, the two Fresnel terms, bsdf_f /
bsdf_pdf / bsdf_sample -- per sample against the fp64 reference of tests/bsdf_reference.py, whose allowance comes from its own sensitivity and
from operation counts (its module docstring), never from this kernel's output.  tests/test_bsdf_reference.py shows on the CPU that the
reference meets closed forms it was not written from, that the oracle stays within the same allowance on the same inputs, and that the
inputs stay within their set-aside caps.

Everything goes through rene_bsdf_eval (Bsdf<5> with every lobe kind; a few thousand lanes of a 64-thread kernel per call, no render), on
two contexts of the shared scene: materials resolved at upload (Inst::res_*) and under RENE_NO_RESOLVE (the material and texture tables).
Every probe runs on both and the two answers are bit-identical.  Per material (32: all seven kinds and None, over Solid, Checkerboard and
ImageMap parameters; alphas 0.25 .. 0.01, anisotropic, remapped, under the 1e-3 clamp; Uber with 1 to 5 lobes) and input set (uniform 2 048,
grazing 1 024, the named edge rows): lobe counts exact; f, pdf, and the sampled wi, f, pdf within the allowance wherever the sample is not
set aside by the reference's own rule (an exemption of an edge row concerns the cap's count alone, which the CPU file asserts); finite wherever
the reference is, and of the reference's class (+-inf, NaN) where it is not -- set-aside samples included.  For the
single-lobe non-specular materials a second probe evaluates f and pdf at the device's own sampled wi: they are the sampled f and pdf to within
the two allowances.

Largest error / allowance observed on an MI355X (a record, not a threshold; the oracle's own on the same inputs in brackets), over f, pdf and
the sampled wi, f, pdf:
  Lambert (Matte, Uber with kd alone)   uniform 0.27 (0.27), grazing 0.27 (0.27), edge 0.27 (0.27) -- the sampled f, one multiply by fp32(1 / pi)
  specular (Glass, Mirror)              uniform 0.33 (0.33), grazing 0.31 (0.34), edge 0.20 (0.22)
  Metal                                 uniform 0.64 (1.00), grazing 0.93 (0.93), edge 0.30 (0.18); the alpha = 0.01 plate's sampled pdf is the 0.93 and
                                        the 1.00: D at a half vector whose 1 - z^2 rounds to 0, which is as far as that clamp lets it go
  Substrate                             uniform 0.26 (0.22), grazing 0.26 (0.22), edge 0.78 (0.78) -- f at a wi one degree off the horizon (`a just below 1.6 for wi, alpha 0.01`)
  Plastic                               uniform 0.28 (0.27), grazing 0.27 (0.27), edge 0.27 (0.27)
  Uber, 2 to 5 lobes                    uniform 0.30 (0.27), grazing 0.27 (0.27), edge 0.27 (0.27)
  sampled against evaluated             0.16 at most
The two contexts agreed bit for bit on every probe; no device or oracle defect was found.  Scratch builds of device_code.inc with one line
reverted each fail here: tr_pdf without the abs -- test_the_edge_rows (pdf of `wi longer than wo and nearly opposite`, the only way to a negative
dot(wo, wh)); fr_dielectric without the index swap -- test_the_uniform_set[glass-1.5]; the Microfacet f without face_forward --
test_the_uniform_set[plastic]; tr_sample_wh without the flip -- test_the_uniform_set[metal-0.25] (no sample below the surface); Plastic with
(1, 1.5) -- test_the_uniform_set[plastic]; bsdf_sample without pdf / len -- test_the_uniform_set[plastic]; cos_phi / sin_phi without their
sin_theta == 0 case -- test_the_edge_rows[metal-0.25] (the sampled wi of `wo == n`).
"""
import numpy as np
import pytest

import bsdf_reference as br
from rene_amd import api

pytestmark = pytest.mark.gpu

S = br.shared_scene()


@pytest.fixture(scope="module")
def contexts():
    """The shared scene on two contexts: materials resolved at upload, and under RENE_NO_RESOLVE (read when the scene is packed)."""
    mp = pytest.MonkeyPatch()
    mp.delenv("RENE_NO_RESOLVE", raising=False)
    resolved = api.Renderer(S.scene)
    mp.setenv("RENE_NO_RESOLVE", "1")
    tables = api.Renderer(S.scene)
    mp.undo()
    yield resolved, tables
    resolved.close()
    tables.close()


def _probe(contexts, case, n, uv, wo, wi, seeds):
    """(n, 12) from the device, the same bits with and without the resolve."""
    g = [r.bsdf_eval(S.material[case], n, uv, wo, wi, seeds) for r in contexts]
    assert np.array_equal(g[0].view(np.uint32), g[1].view(np.uint32)), (case, "the resolved record and the tables differ")
    return g[0]


def _held(contexts, oracle_mod, case, which):
    I = br.input_set(case, which)
    rows = _probe(contexts, case, I.n, I.uv, I.wo, I.wi, I.seeds)
    result, counts = br.check(rows, case, which)
    oracle, _ = br.check(br.oracle_rows(oracle_mod, case, which), case, which)
    print(f"{case} {which}: error / allowance " + ", ".join(f"{q} {result[q][0]:.2f} ({oracle[q][0]:.2f})" for q in br.QUANTITIES))
    assert counts, (case, which, "lobe counts")
    for q, (_, bad) in result.items():
        names = [I.names[i] for i in np.nonzero(bad)[0]] if I.names else np.nonzero(bad)[0][:8]
        assert not bad.any(), (case, which, q, int(bad.sum()), names, rows[bad][:3])
    return rows


@pytest.mark.parametrize("case", br.CASES)
def test_the_uniform_set(case, contexts, oracle_mod):
    _held(contexts, oracle_mod, case, "uniform")


@pytest.mark.parametrize("case", br.CASES)
def test_the_grazing_set(case, contexts, oracle_mod):
    _held(contexts, oracle_mod, case, "grazing")


@pytest.mark.parametrize("case", br.CASES)
def test_the_edge_rows(case, contexts, oracle_mod):
    _held(contexts, oracle_mod, case, "edge")


@pytest.mark.parametrize("case", br.SINGLE_NON_SPECULAR)
def test_sampled_and_evaluated_values_agree(case, contexts):
    """A second probe at the device's own sampled wi: f and pdf there are the sample's f and pdf, to the evaluation's allowance at that wi plus
    the sample's (at most twice the larger).  Samples set aside on either side, and those that drew nothing, are left out."""
    worst = {}
    for which in ("uniform", "grazing"):
        I = br.input_set(case, which)
        first = _probe(contexts, case, I.n, I.uv, I.wo, I.wi, I.seeds)
        s_wi = np.ascontiguousarray(first[:, 4:7])
        second = _probe(contexts, case, I.n, I.uv, I.wo, s_wi, I.seeds)
        _, sm = br.reference(case, which)
        ev = br.evaluate(S.scene, S.material[case], I.n, I.uv, I.wo, s_wi)
        drawn = (first[:, 10] > 0) & (sm.pdf > 0)
        for q, got, want, allow, aside in (("f", second[:, 0:3], first[:, 7:10], ev.f_allow + sm.f_allow, ev.aside["f"] | sm.aside["f"]),
                                           ("pdf", second[:, 3], first[:, 10], ev.pdf_allow + sm.pdf_allow, ev.aside["pdf"] | sm.aside["pdf"])):
            keep = drawn & ~aside
            assert keep.mean() > 0.25, (case, which, q, keep.mean())
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))[keep]
            assert np.isfinite(got[keep]).all() and (err <= allow[keep]).all(), (case, which, q, np.nonzero(keep)[0][(err > allow[keep]).reshape(len(err), -1).any(-1)][:8])
            worst[which, q] = br.tr.ratio(err, allow[keep])
    print(f"{case}: sampled against evaluated, error / allowance " + ", ".join(f"{w} {q} {v:.2f}" for (w, q), v in worst.items()))

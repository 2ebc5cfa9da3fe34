"""Which scenes the packer marks for the emitter-query fusion (csrc/scene_pack.cpp, mark_emit_twin; no GPU): exactly the ones whose emitter
structure is one triangle / parallelogram item with exactly one bit-equal item in the main list."""
import numpy as np
import pytest

from emit_fusion_scenes import block_light, cornell_sun, deep_paths, triangle_light, twin_marks
from rene_amd import abi, scenes
from test_gpu_frame_stream import many_emitters, no_emitters

KIND_QUAD, KIND_TRIANGLE, KIND_BOX = (int(np.float32(v).view(np.uint32)) for v in (0.0, 1.0, 3.0))


@pytest.fixture(autouse=True)
def fusion_default(monkeypatch, hip_lib):
    monkeypatch.delenv("RENE_EMIT_FUSION", raising=False)


def check_twin(scene, kind):
    marked, main, n_main, emit, n_emit = twin_marks(scene)
    assert n_emit == 1 and len(marked) == 1, (marked, n_main, n_emit)
    twin, em = main[marked[0]], emit[0]
    assert np.array_equal(twin[:13], em[:13])  # plane, reciprocal basis and kind: bit for bit
    assert (twin[15] & 0xFFFF) == (em[15] & 0xFFFF) and twin[15] >> 16 == 0x8000  # the perms, and nothing but the mark above them
    assert em[12] == kind
    others = [i for i in range(n_main) if i != marked[0]]
    assert not any(np.array_equal(main[i, :13], em[:13]) for i in others)
    return marked[0], main, n_main


def test_cornell_marks_its_light_quad():
    twin, main, n_main = check_twin(scenes.cornell_box(64, 64), KIND_QUAD)
    assert n_main == 4 and twin == 2
    assert [int(k) for k in main[:n_main, 12]] == [KIND_BOX, KIND_BOX, KIND_QUAD, KIND_BOX]
    assert main[twin, 15] == 0x80000104


@pytest.mark.parametrize("build", [cornell_sun, deep_paths], ids=["cornell_sun", "deep_paths"])
def test_cornell_variants_mark_the_same_quad(build):
    twin, _, n_main = check_twin(build(32, 32), KIND_QUAD)
    assert n_main == 4 and twin == 2


def test_single_triangle_light_marks_a_triangle_twin():
    check_twin(triangle_light(32, 32), KIND_TRIANGLE)


@pytest.mark.parametrize("build", [lambda: many_emitters()[0], lambda: no_emitters()[0], lambda: scenes.veach_mis(64, 36),
                                   lambda: block_light(32, 32)], ids=["many_emitters", "no_emitters", "veach_mis", "block_light"])
def test_everything_else_keeps_the_separate_query(build):
    marked, main, n_main, emit, n_emit = twin_marks(build())
    assert n_main > 0 and marked == []


def test_block_light_is_a_box_in_both_structures():
    _, main, n_main, emit, n_emit = twin_marks(block_light(32, 32))
    assert n_emit == 1 and emit[0, 12] == KIND_BOX  # the light quad went into the block's box item: nothing to pair


def test_the_environment_switch_marks_none(monkeypatch):
    monkeypatch.setenv("RENE_EMIT_FUSION", "0")
    assert twin_marks(scenes.cornell_box(64, 64))[0] == []
    assert twin_marks(triangle_light(32, 32))[0] == []
    monkeypatch.setenv("RENE_EMIT_FUSION", "1")
    assert twin_marks(scenes.cornell_box(64, 64))[0] == [2]

"""CPU: the kernel matrix of tests/kernel_matrix.py reaches every render kernel the build compiles.  Each catalogue entry lands on
the leaf of the dispatch it is there for (rene_pack_info, no GPU), and the kernels that kernel_matrix.expected_kernel names for the
entries and their variants are exactly the render_kernel / render_kernel_wf instantiations listed in rene_amd/csrc/<unit>.res: a
new instantiation without a catalogue entry fails here.  test_gpu_kernel_matrix.py checks expected_kernel against the launch log."""
import pytest

import kernel_matrix as km
from rene_amd import api


@pytest.mark.parametrize("name", [e.name for e in km.CATALOGUE])
def test_each_entry_lands_on_its_leaf(hip_lib, name):
    e = km.BY_NAME[name]
    info = api.pack_info(e.build())
    assert (info.features & km.VOLPATH != 0) == e.family.startswith("vol")
    if e.family.endswith("item"):
        assert info.features & km.SMALL
    else:  # deep enough a tree for the traversal-restart kernel
        assert not info.features & km.SMALL and info.n_nodes_main > km.RESTART_MIN_NODES
    for v in km.VARIANTS[e.family]:
        k = km.expected_kernel(info, v.flags, v.no_lds_tables)
        assert ("render_kernel_wf" in k) == (e.family.endswith("restart") and not v.flags & km.abi.FLAG_NO_RESTART), (v.name, k)
        if not v.flags & km.abi.FLAG_NO_RESTART:
            assert km.kernel_feat(k) == e.leaf, (v.name, k)
    if name == "matte+emissive-mesh":  # the emitter-only structure is deep as well
        assert info.n_nodes_emit > km.RESTART_MIN_NODES and info.emit_object_len > 0


def test_the_catalogue_covers_every_render_kernel_of_the_build(hip_lib):
    res = km.res_kernel_names()
    if res is None:
        pytest.skip("rene_amd/csrc/*.res missing: build with `make -C rene_amd/csrc` (the Makefile writes them)")
    got = {km.expected_kernel(api.pack_info(e.build()), v.flags, v.no_lds_tables) for e in km.CATALOGUE for v in km.VARIANTS[e.family]}
    assert got == res, {"not reached": sorted(res - got), "not compiled": sorted(got - res)}

"""The two forms of the box item's slab evaluation (csrc/box_slabs.h) against each other on the device the tests run on
(csrc/selftest/box_slabs_probe.hip): the dot products on the vector pipe and on the matrix pipe, on Cornell's box records and a few thousand
rays -- random, parallel to a slab, from a face, hitting at tmin, with +-0 components -- with every lane live and with an irregular half of
them dead: c0, c1, t_in, t_out, the accept decision and the hit parameter bit for bit.  CPU: the records are still what the packer makes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from rene_amd import api, scenes

BIN = os.path.join(ROOT, "rene_amd", "csrc", "selftest", "box_slabs_probe")
RECORDS = os.path.join(GOLDEN, "cornell_small_items.npy")
BOX_KIND_BITS = 0x40400000  # 3.0f


def test_the_recorded_items_are_cornells(hip_lib):
    want, n_loop = api.small_items(scenes.cornell_box(64, 64), 0)
    got = np.load(RECORDS)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    kinds = got[:n_loop, 12]
    assert n_loop == 4 and (kinds == BOX_KIND_BITS).sum() == 3  # the room and the two blocks; the fourth item is the light
    assert sorted(got[:n_loop, 14][kinds == BOX_KIND_BITS]) == [0, 0, 2]  # one open face (the room's), two closed boxes


@pytest.mark.gpu
def test_matrix_and_vector_forms_give_the_same_bits():
    assert os.path.exists(BIN), "build it: make -C rene_amd/csrc"
    p = subprocess.run([BIN, RECORDS], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr)
    runs = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()[:2]]
    assert p.returncode == 0 and len(runs) == 2, (p.returncode, p.stdout, p.stderr)
    (all_n, all_bad), (half_n, half_bad) = runs
    assert all_bad == 0 and half_bad == 0, p.stdout
    assert all_n == 4096 * 3 * 10  # every ray against the three boxes, ten values each
    assert 0.4 * all_n < half_n < 0.6 * all_n  # an irregular half of the lanes had no ray

"""CPU: what the work-item switch of the Matte small-scene kernels rests on (rene_amd/csrc/item_slot.h; device_code.inc, RENE_ITEM_SWITCH).
selftest/item_slot_check walks every slot of every owned tile of films from 1 x 1 to 16384 x 16384, ragged ones included, for tile shard counts
1, 2, 3, 5 and 8 and every rank, and counts where the slot a lane keeps is not the slot pixel_slot() rebuilds from the pixel, and where the tile
division of the take (udiv_small, through the host's reciprocal) is not the integer quotient and remainder."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
CHECK = os.path.join(CSRC, "selftest", "item_slot_check")


def test_no_slot_and_no_tile_mismatch(hip_lib):
    if not os.path.exists(CHECK):  # (the library was built by hand: `make` builds this with it)
        subprocess.check_call(["make", "-C", CSRC, "selftest/item_slot_check"])
    p = subprocess.run([CHECK], capture_output=True, text=True)
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and lines[-1] == "mismatches 0", p.stdout
    films = [l for l in lines if l.startswith("film ")]
    assert any(l.startswith("film 1x1 ") for l in films) and any(l.startswith("film 16384x16384 tiles=262144 ") for l in films)
    assert all(l.endswith("mismatches=0") for l in films)

"""CPU: the words of the calls that hand out a library-owned result -- rene_export_features, rene_output_8bit, rene_output_tonemapped, rene_gbuffer,
the four rene_*_buffer getters and the four rene_download_* calls -- where they are refused before a context is looked at.  The strings are
literal: callers match on them, and the calls share their code (Result, result_buffer, result_download in rene_hip.cpp), so a change of one
wording shows here.  tests/test_gpu_result_buffers.py has the refusals that need a context."""
import ctypes as C

import numpy as np
import pytest

GETTERS = ("rene_features_buffer", "rene_output_buffer", "rene_gbuffer_buffer", "rene_denoise_shard_buffer")
DOWNLOADS = ("rene_download_features", "rene_download_output", "rene_download_gbuffer", "rene_download_denoise_shard")
PRODUCERS = ("rene_export_features", "rene_output_8bit", "rene_output_tonemapped", "rene_gbuffer")


def refused(L, rc, text):
    assert rc == -1 and L.rene_last_error() == text.encode(), (rc, L.rene_last_error())


@pytest.mark.parametrize("fn", GETTERS)
def test_a_getter_without_a_context_or_an_argument(hip_lib, fn):
    L = hip_lib
    ptr, n = C.c_void_p(0x1234), C.c_size_t(77)
    refused(L, getattr(L, fn)(None, C.byref(ptr), C.byref(n)), fn + ": NULL argument")
    refused(L, getattr(L, fn)(None, None, C.byref(n)), fn + ": NULL argument")
    refused(L, getattr(L, fn)(None, C.byref(ptr), None), fn + ": NULL argument")
    refused(L, getattr(L, fn)(None, None, None), fn + ": NULL argument")
    assert (ptr.value, n.value) == (0x1234, 77)  # a refused call writes nothing


@pytest.mark.parametrize("fn", DOWNLOADS)
def test_a_download_without_a_context_or_a_destination(hip_lib, fn):
    L = hip_lib
    dst = np.full(64, 0xAB, np.uint8)
    refused(L, getattr(L, fn)(None, dst.ctypes.data_as(C.c_void_p), dst.nbytes), fn + ": NULL argument")
    refused(L, getattr(L, fn)(None, None, 0), fn + ": NULL argument")
    refused(L, getattr(L, fn)(None, None, dst.nbytes), fn + ": NULL argument")
    assert (dst == 0xAB).all()


@pytest.mark.parametrize("fn", PRODUCERS)
def test_a_producing_call_without_a_context(hip_lib, fn):
    L = hip_lib
    dst = np.full(64, 0xAB, np.uint8)
    # (NULL parameters are the defaults, which are valid: the context is what is missing)
    refused(L, getattr(L, fn)(None, None, None, 0), fn + ": NULL context")
    refused(L, getattr(L, fn)(None, None, dst.ctypes.data_as(C.c_void_p), dst.nbytes), fn + ": NULL context")
    assert (dst == 0xAB).all()


def test_a_producing_call_with_its_own_default_parameters(hip_lib):
    from rene_amd import api
    L = hip_lib
    for fn, p in (("rene_export_features", api.feature_params_default()), ("rene_output_8bit", api.output_params_default()),
                  ("rene_output_tonemapped", api.tonemap_params_default()), ("rene_gbuffer", api.gbuffer_params_default())):
        refused(L, getattr(L, fn)(None, C.byref(p), None, 0), fn + ": NULL context")

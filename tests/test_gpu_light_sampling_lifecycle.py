"""The light table of fh_set_light_sampling lives in DeviceBuffer members of the context (csrc/context.h): with the switch on -- the table built, rebuilt for another
scene and for moved instances -- fh_kat_live_allocations is back at its starting values after the context is destroyed.  Beside tests/test_gpu_context_lifecycle.py."""
import ctypes as C

import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes

pytestmark = pytest.mark.gpu


def live():
    count, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert N.lib().fh_kat_live_allocations(C.byref(count), C.byref(nbytes)) == N.FH_OK
    return int(count.value), int(nbytes.value)


def test_a_context_with_light_sampling_on_gives_back_all_it_took():
    before = live()
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        w, h = 32, 24
        cam = F.Camera(**scenes.CORNELL_CAMERA)
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        without = live()
        r.set_light_sampling()
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        with_table = live()
        assert with_table[0] >= without[0] + 5 and with_table[1] > without[1]  # (the table's five buffers, and whatever a second call makes)
        r.set_transforms(*scenes.instanced_transforms((-0.19, 0.0, 0.0)))
        r.build_ias()
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        assert live()[0] >= with_table[0]
        r.load_scene(scenes.textured_cornell_box())  # (more faces: the per-face array is made again)
        r.build_ias()
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        assert live()[0] >= with_table[0]
        r.clear_light_sampling()
    finally:
        r.close()
    assert live() == before

"""The proxies of fh_set_light_resampling live in a DeviceBuffer member of the context beside the light table's (csrc/context.h): with both switches on -- table and
proxies built, rebuilt for another scene and for moved instances -- fh_kat_live_allocations is back at its starting values after the context is destroyed.  Beside
tests/test_gpu_light_sampling_lifecycle.py and tests/test_gpu_context_lifecycle.py."""
import pytest

import fredholm_amd as F
from fredholm_amd import scenes
from test_gpu_light_sampling_lifecycle import live

pytestmark = pytest.mark.gpu


def test_a_context_with_light_resampling_on_gives_back_all_it_took():
    before = live()
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        w, h = 32, 24
        cam = F.Camera(**scenes.CORNELL_CAMERA)
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        r.set_light_resampling(16)  # without light sampling: nothing is built
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        without = live()
        r.set_light_sampling()
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        with_table = live()
        assert with_table[0] >= without[0] + 6 and with_table[1] > without[1]  # (the table's five buffers and the proxies, and whatever a second call makes)
        steady = with_table  # (a context keeps allocating over its first calls -- one path pool per pass in flight: render until a call makes nothing)
        for _ in range(8):
            r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
            r.wait_for_completion()
            steady, last = live(), steady
            if steady == last:
                break
        assert steady == last
        r.set_light_resampling(2)  # M alone: nothing is made or freed
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        assert live() == steady
        r.set_transforms(*scenes.instanced_transforms((-0.19, 0.0, 0.0)))
        r.build_ias()
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        assert live()[0] >= with_table[0]
        r.load_scene(scenes.textured_cornell_box())  # (more faces and other emitters: the arrays are made again)
        r.build_ias()
        r.render(cam, (0.0, 0.0, 0.0), L, 2, 4)
        r.wait_for_completion()
        assert live()[0] >= with_table[0]
        r.clear_light_resampling()
        r.clear_light_sampling()
    finally:
        r.close()
    assert live() == before

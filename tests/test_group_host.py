"""CPU tests of the group interface (include/fredholm_hip.h: fh_ctx_create_group): the exported symbols and their ctypes signatures, the refusals that need no GPU,
the shard layout of the gather against distributed.tile_ownership, FH_DEVICES in the C++ facade and --devices in the batch driver.  What a group renders is
tested on the GPU (test_gpu_group.py)."""
import ctypes as C
import os
import subprocess

import pytest

from fredholm_amd import distributed as D
from fredholm_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fh_ctx_create_group", "fh_ctx_group_size", "fh_ctx_member", "fh_group_set_gather_layers", "fh_group_gather_times", "fh_group_shard_layout")
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
LAYER_BYTES = (16, 16, 4, 16, 16, 16)  # beauty, position, depth, normal, texcoord, albedo: bit k of the gather mask


def test_new_symbols_are_declared_exported_and_prototyped():
    L = N.load_library()
    hdr = open(os.path.join(ROOT, "include", "fredholm_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert fn.argtypes == N.SIGNATURES[name], name
    for name, bit in (("BEAUTY", 1), ("POSITION", 2), ("DEPTH", 4), ("NORMAL", 8), ("TEXCOORD", 16), ("ALBEDO", 32), ("ALL", 63)):
        assert f"#define FH_LAYER_{name} {bit}u" in hdr
        assert getattr(N, "LAYER_" + name) == bit


def _create(devices, n, with_out=True):
    L = N.load_library()
    ctx = C.c_void_p(0xDEAD)
    arr = None if devices is None else (C.c_int * max(len(devices), 1))(*devices)
    rc = L.fh_ctx_create_group(arr, n, C.byref(ctx) if with_out else None)
    msg = L.fh_last_error(None)
    return rc, (msg or b"").decode(), ctx


@pytest.mark.parametrize("devices,n", [(None, 2), ([0, 0], 0), ([0] * 17, 17)])
def test_bad_groups_are_refused_without_a_gpu(devices, n):
    rc, msg, ctx = _create(devices, n)
    assert rc == -1  # FH_E_INVALID
    assert "fh_ctx_create_group" in msg
    assert ctx.value is None  # *out is cleared: nothing half-made is handed back


def test_null_out_is_refused_without_a_gpu():
    rc, msg, _ = _create([0, 0], 2, with_out=False)
    assert rc == -1 and "fh_ctx_create_group" in msg


def _owned(w, h, r, n, tw, th):
    return D.tile_ownership(w, h, r, n, tw, th).size


@pytest.mark.parametrize("w,h,n,tw,th", [(64, 48, 2, 32, 32), (70, 50, 3, 16, 8), (1920, 1080, 8, 32, 32), (5, 5, 4, 32, 32), (40, 40, 16, 32, 32), (33, 31, 2, 32, 32)])
@pytest.mark.parametrize("mask", [N.LAYER_ALL, N.LAYER_BEAUTY, N.LAYER_DEPTH, N.LAYER_BEAUTY | N.LAYER_DEPTH | N.LAYER_ALBEDO])
def test_shard_layout_follows_the_tile_ownership(w, h, n, tw, th, mask):
    """a member's shard is its owned pixels of the selected layers, layer after layer, each padded to 16 bytes; the lead packs nothing"""
    got = N.group_shard_layout(w, h, n, mask, tw, th)
    want = [0, 0]
    for r in range(1, n):
        owned = _owned(w, h, r, n, tw, th)
        want.append(want[-1] + sum((owned * LAYER_BYTES[k] + 15) // 16 * 16 for k in range(6) if mask >> k & 1))
    assert got == want
    assert sum(_owned(w, h, r, n, tw, th) for r in range(n)) == w * h
    if mask == N.LAYER_ALL:  # at most 84 bytes per owned pixel (plus the padding of the one 4-byte layer)
        assert all(b - a <= 84 * _owned(w, h, r, n, tw, th) + 12 for r, (a, b) in enumerate(zip(got, got[1:])))


def test_shard_layout_refuses_bad_arguments():
    L = N.load_library()
    out = (C.c_uint64 * 18)()
    for args in ((0, 8, 32, 32, 2, 63), (8, 8, 0, 32, 2, 63), (8, 8, 32, 32, 0, 63), (8, 8, 32, 32, 17, 63), (8, 8, 32, 32, 2, 64), (70000, 8, 32, 32, 2, 63)):
        assert L.fh_group_shard_layout(*args, out) == -1, args
    assert L.fh_group_shard_layout(8, 8, 32, 32, 2, 63, None) == -1


_FACADE = """
#include "fredholm/renderer.h"
#include <cstdio>
int main()
{
  try {
    optwl::Context context;
    fredholm::Renderer renderer(context.get_context());
    renderer.set_gather_layers(FH_LAYER_BEAUTY | FH_LAYER_ALBEDO);
    std::printf("group of %u\\n", renderer.group_size());
  } catch (const std::exception& e) {
    std::printf("threw: %s\\n", e.what());
    return 3;
  }
  return 0;
}
"""


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_facade_reads_fh_devices(tmp_path):
    src = tmp_path / "group_facade.cpp"
    src.write_text(_FACADE)
    exe = tmp_path / "group_facade"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), *LINK, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(value):
        env = {k: v for k, v in os.environ.items() if k != "FH_DEVICES"}
        if value is not None:
            env["FH_DEVICES"] = value
        return subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)

    for bad in ("0,x", ",", "0,-1", "", "0,,1", "0;1"):  # unparsable: an exception that names the variable, never a silent device 0
        p = run(bad)
        assert p.returncode == 3 and "FH_DEVICES" in p.stdout, (bad, p.stdout, p.stderr)
    for plain in (None, "0"):  # today's call: a plain context, or on a machine without a GPU its error
        p = run(plain)
        assert "FH_DEVICES" not in p.stdout, (plain, p.stdout)
        if _no_gpu():
            assert p.returncode == 3 and "no HIP device" in p.stdout, (plain, p.stdout)
        else:
            assert p.returncode == 0 and "group of 1" in p.stdout, (plain, p.stdout, p.stderr)
    p = run("0,0")  # parsed: the group call, which needs a GPU
    assert "FH_DEVICES" not in p.stdout
    if _no_gpu():
        assert p.returncode == 3 and "no HIP device" in p.stdout
    else:
        assert p.returncode == 0 and "group of 2" in p.stdout, (p.stdout, p.stderr)


def test_rtcamp_builds_with_the_devices_flag(tmp_path):
    exe = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    usage = subprocess.run([str(exe)], capture_output=True, text=True)
    assert usage.returncode == 2 and "--devices" in usage.stderr
    bad = subprocess.run([str(exe), "--scene", "x.obj", "--devices", "0,x"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--devices" in bad.stderr


def test_python_renderer_takes_a_device_list():
    import fredholm_amd as F
    with pytest.raises(F.FredholmError) as e:
        F.Renderer(devices=[])
    assert "fh_ctx_create_group" in str(e.value)
    with pytest.raises(F.FredholmError):
        F.Renderer(devices=[0] * 17)

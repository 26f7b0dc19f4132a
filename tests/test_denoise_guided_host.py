"""CPU tests of the variance-guided denoiser's interface (include/fredholm_hip.h: fh_denoise_guided): the exported symbol and its ctypes signature, the layout of
its two structs, its refusals -- which are decided from the arguments alone, before the context or the device is touched -- and the Python facade.  The filter
itself is tested on the GPU (test_gpu_denoise_guided.py)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

from fredholm_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FH_E_INVALID = -1


def test_symbol_is_exported_with_its_signature():
    L = N.load_library()
    assert "fh_denoise_guided" in N.EXPORTS
    fn = L.fh_denoise_guided
    assert fn.restype is C.c_int
    assert fn.argtypes == N.SIGNATURES["fh_denoise_guided"] == [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(N.DenoiseInputsC), C.POINTER(N.DenoiseParamsC), C.c_void_p, C.c_int]
    hdr = open(os.path.join(ROOT, "include", "fredholm_hip.h")).read()
    assert ("int fh_denoise_guided(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* inputs, const fh_denoise_params* params, float* denoised, "
            "int upscale2x);") in hdr


def test_structs_have_the_header_layout(tmp_path):
    inputs = ("beauty", "normal", "albedo", "position", "depth", "moments", "counts")
    params = ("sigma_l", "sigma_z", "sigma_a", "normal_power_log2", "passes")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) {\n  printf("%zu %zu\\n", sizeof(fh_denoise_inputs), sizeof(fh_denoise_params));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(fh_denoise_inputs, {f}));\n' for f in inputs)
                   + "".join(f'  printf("%zu\\n", offsetof(fh_denoise_params, {f}));\n' for f in params) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    I, P = N.DenoiseInputsC, N.DenoiseParamsC
    assert [name for name, _ in I._fields_] == list(inputs) and [name for name, _ in P._fields_] == list(params)
    want = [C.sizeof(I), C.sizeof(P)] + [getattr(I, f).offset for f in inputs] + [getattr(P, f).offset for f in params]
    assert got == want == [56, 20, 0, 8, 16, 24, 32, 40, 48, 0, 4, 8, 12, 16]


def _call(ctx, ptrs, params, w=8, h=8, dst=1 << 20):
    i = N.DenoiseInputsC(*ptrs)
    rc = N.lib().fh_denoise_guided(ctx, w, h, C.byref(i), None if params is None else C.byref(N.DenoiseParamsC(*params)), dst, 0)
    return rc, N.lib().fh_last_error(None).decode()


def test_every_refusal_is_decided_before_the_context_is_touched():
    """the pointers below are never dereferenced: a refused call returns before it looks at the context (here NULL: no GPU is needed), and a call whose arguments
    are in order gets as far as the context check, which is the only thing left to refuse it"""
    full = [0x1000 * (k + 1) for k in range(7)]  # (made-up device addresses)
    ok = (2.0, 1.0, 0.2, 7, 5)
    for params in (ok, None, (0.5, 4.0, 1.0, 0, 1), (0.5, 4.0, 1.0, 10, 6)):
        rc, msg = _call(None, full, params)
        assert rc == FH_E_INVALID and msg == "fh_denoise_guided: null context", (params, msg)
    for pair in ((3, 4), (5, 6)):  # whole pairs may be absent
        ptrs = [None if k in pair else p for k, p in enumerate(full)]
        assert _call(None, ptrs, ok)[1] == "fh_denoise_guided: null context"
    assert _call(None, full[:3] + [None] * 4, ok)[1] == "fh_denoise_guided: null context"
    refused = []
    for k in range(3):  # a missing required pointer
        refused.append(([None if j == k else p for j, p in enumerate(full)], ok, "required"))
    for k in (3, 4):  # half a pair
        refused.append(([None if j == k else p for j, p in enumerate(full)], ok, "position and depth"))
    for k in (5, 6):
        refused.append(([None if j == k else p for j, p in enumerate(full)], ok, "moments and counts"))
    for k in range(3):
        for v in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            refused.append((full, ok[:k] + (v,) + ok[k + 1:], "sigma"))
    refused += [(full, (2.0, 1.0, 0.2, 11, 5), "normal_power_log2"), (full, (2.0, 1.0, 0.2, 7, 0), "passes"), (full, (2.0, 1.0, 0.2, 7, 7), "passes")]
    for ptrs, params, word in refused:
        rc, msg = _call(None, ptrs, params)
        assert rc == FH_E_INVALID and msg.startswith("fh_denoise_guided: ") and word in msg and "null context" not in msg, (ptrs, params, msg)
    for kw, word in ((dict(dst=None), "null argument"), (dict(w=0), "width"), (dict(h=0), "width"), (dict(w=32769), "width")):
        rc, msg = _call(None, full, ok, **kw)
        assert rc == FH_E_INVALID and word in msg, (kw, msg)
    assert N.lib().fh_denoise_guided(None, 8, 8, None, None, 1 << 20, 0) == FH_E_INVALID and "null argument" in N.lib().fh_last_error(None).decode()


def test_python_facade_has_the_method_with_the_library_defaults():
    from fredholm_amd.renderer import Renderer
    sig = inspect.signature(Renderer.denoise_guided)
    d = {p.name: p.default for p in sig.parameters.values()}
    assert [d[k] for k in ("sigma_l", "sigma_z", "sigma_a", "normal_power_log2", "passes", "upscale")] == [2.0, 1.0, 0.2, 7, 5, False]
    assert [d[k] for k in ("position_ptr", "depth_ptr", "moments_ptr", "counts_ptr")] == [None] * 4
    assert np.float32(d["sigma_a"]) == np.float32(0.2)

"""Caller-supplied rays without a GPU (include/mi355rt.h, "caller-supplied rays"): the two entry points, the constants and the layout of
mi355rt_ray_outputs exist as the header states them, the ctypes mirror agrees with the C compiler, and the Python wrappers refuse bad arguments
before any library call (they are tried on an object with no handle at all: a call that reached the library would fail differently)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355rt.h")


def test_the_two_symbols_and_the_constants_exist(pkg):
    lib = pkg.lib()
    assert hasattr(lib, "mi355rt_trace_rays") and hasattr(lib, "mi355rt_render_rays")
    names = {n: (res, args) for n, res, args in pkg.ABI}
    assert len(names["mi355rt_trace_rays"][1]) == 6 and len(names["mi355rt_render_rays"][1]) == 6
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+MI355RT_RAYS_HOST\s+0u", text) and re.search(r"#define\s+MI355RT_RAYS_DEVICE\s+1u", text)
    assert (pkg.RAYS_HOST, pkg.RAYS_DEVICE) == (0, 1)
    assert re.search(r"int\s+mi355rt_trace_rays\s*\(\s*mi355rt_handle\s*\*[^,]*,\s*const\s+float\s*\*[^,]*,\s*const\s+uint32_t\s*\*[^,]*,\s*size_t[^,]*,\s*uint32_t[^,]*,"
                     r"\s*const\s+mi355rt_ray_outputs\s*\*[^)]*\)\s*;", text)
    assert re.search(r"int\s+mi355rt_render_rays\s*\(\s*mi355rt_handle\s*\*[^,]*,\s*const\s+float\s*\*[^,]*,\s*size_t[^,]*,\s*uint32_t[^,]*,\s*uint32_t[^,]*,"
                     r"\s*mi355rt_ray_counts\s*\*[^)]*\)\s*;", text)


def test_ray_outputs_layout_matches_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u %u\\n",sizeof(mi355rt_ray_outputs),'
                   'offsetof(mi355rt_ray_outputs,rgb),offsetof(mi355rt_ray_outputs,direct),offsetof(mi355rt_ray_outputs,tuv),offsetof(mi355rt_ray_outputs,prim),'
                   'MI355RT_RAYS_HOST,MI355RT_RAYS_DEVICE);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = pkg.RayOutputs
    assert got == [C.sizeof(R), R.rgb.offset, R.direct.offset, R.tuv.offset, R.prim.offset, pkg.RAYS_HOST, pkg.RAYS_DEVICE]
    assert [n for n, _ in R._fields_] == list(pkg.RAY_OUTPUTS) == ["rgb", "direct", "tuv", "prim"]


def test_null_handle_calls_are_refused(pkg):
    lib = pkg.lib()
    rays = np.zeros((1, 6), np.float32)
    out = pkg.RayOutputs()
    assert lib.mi355rt_trace_rays(None, rays.ctypes.data, None, 1, 0, C.byref(out)) == -1
    assert lib.mi355rt_render_rays(None, rays.ctypes.data, 1, 1, 0, None) == -1


class _NoHandle:
    """what a wrapper method needs before it reaches the library; _h is None, so a library call would be a null-handle call, and _check raises something
    no argument check raises"""
    width, height, _h = 4, 3, None

    def _check(self, code):
        raise AssertionError("the library was called (code %d)" % code)


@pytest.fixture()
def nohandle(pkg):
    class T(_NoHandle):
        trace_rays = pkg.RayTracer.trace_rays
        render_rays = pkg.RayTracer.render_rays
    return T()


def test_trace_rays_argument_errors_are_raised_before_any_library_call(nohandle):
    ok = np.zeros((5, 6), np.float32)
    with pytest.raises(TypeError, match="rays6.*dtype"):
        nohandle.trace_rays(ok.astype(np.float64))
    with pytest.raises(ValueError, match="rays6.*shape"):
        nohandle.trace_rays(np.zeros((5, 5), np.float32))
    with pytest.raises(ValueError, match="rays6.*shape"):
        nohandle.trace_rays(np.zeros(30, np.float32))
    with pytest.raises(ValueError, match="rays6.*contiguous"):
        nohandle.trace_rays(np.zeros((5, 12), np.float32)[:, ::2])
    with pytest.raises(TypeError, match="rays6"):
        nohandle.trace_rays([[0.0] * 6])
    with pytest.raises(TypeError, match="keys.*dtype"):
        nohandle.trace_rays(ok, keys=np.zeros((5, 2), np.int64))
    with pytest.raises(ValueError, match="keys.*shape"):
        nohandle.trace_rays(ok, keys=np.zeros((4, 2), np.uint32))
    with pytest.raises(ValueError, match="keys.*contiguous"):
        nohandle.trace_rays(ok, keys=np.zeros((5, 4), np.uint32)[:, ::2])
    for want in ((), ("colour",), ("rgb", "rgb")):
        with pytest.raises(ValueError, match="want"):
            nohandle.trace_rays(ok, want=want)


def test_render_rays_argument_errors_are_raised_before_any_library_call(nohandle):
    npix = nohandle.width * nohandle.height
    with pytest.raises(ValueError, match="spp"):
        nohandle.render_rays(np.zeros((npix, 6), np.float32), 0)
    with pytest.raises(ValueError, match="rays6.*shape"):
        nohandle.render_rays(np.zeros((npix * 2 - 1, 6), np.float32), 2)
    with pytest.raises(TypeError, match="rays6.*dtype"):
        nohandle.render_rays(np.zeros((npix, 6), np.float64), 1)
    with pytest.raises(ValueError, match="rays6.*contiguous"):
        nohandle.render_rays(np.zeros((npix, 12), np.float32)[:, ::2], 1)


def test_cpu_tensors_and_wrong_tensor_dtypes_are_refused_in_python(nohandle):
    import torch
    with pytest.raises(ValueError, match="GPU"):
        nohandle.trace_rays(torch.zeros((5, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="GPU"):
        nohandle.render_rays(torch.zeros((12, 6), dtype=torch.float32), 1)

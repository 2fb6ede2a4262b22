"""The histogram kernel source (backend/hip.py ``JitHistogram``) for
float64 and float32 fields, in the LDS template and the global-atomics
template: generated with ``compile=False`` and inspected without a
device, and cross-compiled for gfx950 where hipcc is present.

A float32 field must be read through ``const real*`` with ``using real =
float``; the bins (``lh``, ``hist``) stay double and each weight is
widened where it is added.
"""

import os
import re
import shutil
import subprocess

import pytest
import torch

from pystella_amd.backend import hip
from pystella_amd.field import Field, get_field_args, var

RANK_SHAPE = (70, 11, 72)
H = 2
DTYPES = {"float64": torch.float64, "float32": torch.float32}
RTYPE = {"float64": "double", "float32": "float"}


def _pairs(num_bins):
    F = Field("f", offset="h")
    G = Field("g", offset=0)
    return [(F * num_bins, 1), (G * num_bins, F),
            ((1 - G) * num_bins, F * F * var("c"))]


# 3 x 64 doubles fit the LDS bins; 3 x 4096 do not
TEMPLATES = {"lds": 64, "global": 4096}


def _kernel(template, dtype):
    num_bins = TEMPLATES[template]
    pairs = _pairs(num_bins)
    exprs = [e for pair in pairs for e in pair]
    return hip.JitHistogram(
        pairs, num_bins, get_field_args(exprs), ["c"], (H,) * 3,
        RANK_SHAPE, dtype=DTYPES[dtype], compile=False)


def _params(src, name="hist_map"):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


CASES = [(t, d) for t in TEMPLATES for d in DTYPES]


@pytest.fixture
def no_native_module(monkeypatch):
    def no_ext():
        raise AssertionError("compile=False touched the native module")
    monkeypatch.setattr(hip, "ext", no_ext)


@pytest.mark.parametrize("template,dtype", CASES)
def test_source_reads_fields_in_their_own_type(template, dtype,
                                               no_native_module):
    k = _kernel(template, dtype)
    assert k.key is None and k.dtype == DTYPES[dtype]
    src = k.source
    assert src.count("using real =") == 1
    assert f"using real = {RTYPE[dtype]};" in src
    params = _params(src)
    assert params == ["const real* __restrict__ f",
                      "const real* __restrict__ g",
                      "double* __restrict__ hist", "double s_c"]
    # no pointer parameter names a concrete field type
    assert not re.search(r"(double|float)\s*\*\s*(__restrict__\s*)?[fg]\b",
                         src)
    # the bins are double and every weight is widened where it is added
    adds = re.findall(r"atomicAdd\(&lh\[(\d) \* NBINS \+ bb\], (.*?)\); \}",
                      src)
    assert [a for a, _ in adds] == ["0", "1", "2"]
    assert all(w.startswith("(double)(") for _, w in adds)
    if template == "lds":
        assert "__shared__ double lh[NHIST * NBINS];" in src
        assert "atomicAdd(&hist[b], lh[b]);" in src
    else:
        assert "double* lh = hist;" in src
        assert "__shared__" not in src
    assert f"#define NBINS {TEMPLATES[template]}" in src
    assert "#define NHIST 3" in src


@pytest.mark.parametrize("template", list(TEMPLATES))
def test_float_and_double_sources_differ_only_in_real(template,
                                                      no_native_module):
    s64 = _kernel(template, "float64").source
    s32 = _kernel(template, "float32").source
    assert s64 != s32
    assert s32.replace("using real = float;", "using real = double;") == s64


def test_source_only_kernel_refuses_to_launch(no_native_module):
    k = _kernel("lds", "float32")
    with pytest.raises(RuntimeError):
        k({})


def test_default_dtype_is_float64(no_native_module):
    pairs = _pairs(64)
    exprs = [e for pair in pairs for e in pair]
    k = hip.JitHistogram(pairs, 64, get_field_args(exprs), ["c"],
                         (H,) * 3, RANK_SHAPE, compile=False)
    assert k.dtype == torch.float64
    assert "using real = double;" in k.source


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_sources_compile_for_gfx950(tmp_path):
    """Device-only cross-compilation of all four sources."""
    procs = []
    for template, dtype in CASES:
        form = f"{template}_{dtype}"
        path = tmp_path / f"{form}.hip"
        path.write_text(_kernel(template, dtype).source)
        procs.append((form, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-std=c++17", "-ffp-contract=fast",
             "-include", "hip/hip_runtime.h",
             "-c", str(path), "-o", str(tmp_path / f"{form}.co")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for form, proc in procs:
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (form, out[-3000:])
        assert (tmp_path / f"{form}.co").stat().st_size > 0

"""The complex64 forms of the observable k-space kernels (backend/hip.py
``projector_source`` and ``spectra_bin_source`` with
``ctype="complex64"``): every source generated and inspected without a
device and cross-compiled for gfx950 where hipcc is present; the
complex128 forms, which must not change; and the float32 CPU classes,
which never reach a kernel, against the end-to-end bound the GPU tests
use.
"""

import difflib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pystella_amd.backend import hip
from tests.obs_c64_reference import (
    KSHAPE, assert_end_to_end, run_spectra)

# (op, times_abs_k): the seven kernels, both forms of the two that
# divide or multiply by |k|
VARIANTS = [("transversify", False), ("vec_to_pol", False),
            ("pol_to_vec", False), ("decompose_vector", False),
            ("decompose_vector", True), ("decomp_to_vec", False),
            ("decomp_to_vec", True), ("tensor_to_pol", False),
            ("pol_to_tensor", False)]
IDS = [f"{op}{'-abs_k' if tak else ''}" for op, tak in VARIANTS]

# name of each written parameter -> components stored
WRITTEN = {"transversify": {"out": 3}, "vec_to_pol": {"plus": 1, "minus": 1},
           "pol_to_vec": {"out": 3},
           "decompose_vector": {"plus": 1, "minus": 1, "lngp": 1},
           "decomp_to_vec": {"out": 3},
           "tensor_to_pol": {"plus": 1, "minus": 1},
           "pol_to_tensor": {"hij": 6}}


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _float_uses(src):
    """Every appearance of the token ``float`` with what follows it."""
    return re.findall(r"\bfloat\b\s*\S?", src)


def test_there_are_seven_kernels():
    assert len({op for op, _ in VARIANTS}) == 7 == len(WRITTEN)


@pytest.mark.parametrize("op,tak", VARIANTS, ids=IDS)
def test_projector_c64_source(op, tak):
    src = hip.projector_source(op, KSHAPE, tak, ctype="complex64")
    assert src == hip.projector_source(op, KSHAPE, tak,
                                       ctype=torch.complex64)
    assert f"#define TIMES_ABS_K {int(tak)}\n" in src
    assert "#define NKX 12\n#define NKY 10\n#define NKZ 8\n" in src
    params = _params(src, f"proj_{op}_c64")
    data = [p for p in params if not p.startswith("const double*")]
    assert data and all(p.startswith("float2* __restrict__ ") for p in data)
    assert params[-3:] == ["const double* __restrict__ eff_x",
                           "const double* __restrict__ eff_y",
                           "const double* __restrict__ eff_z"]
    assert len(data) + 3 == len(params)
    # cplx is a struct of doubles, and nothing per site is a float: the
    # token appears only as the cast of a store's two parts
    assert "struct cplx { double x; double y; };" in src
    assert _float_uses(src) == ["float)", "float)"]
    assert "make_float2((float)(v).x, (float)(v).y)" in src
    assert not re.search(r"\bfloat2\s+\w+\s*[=;]", src.split(
        'extern "C"')[1]), "a float2 variable in the kernel body"
    # one 8-byte access per mode
    assert "#define LDC(p, c) widen((p)[(long)(c)*VOLK + idx])" in src
    # exactly one store per output component, all after the last load
    body = src.split('extern "C"')[1]
    stores = re.findall(r"STC\((\w+),(\d),", body)
    want = [(name, str(c)) for name, n in WRITTEN[op].items()
            for c in range(n)]
    assert sorted(stores) == sorted(want)
    assert body.rindex("LDC(") < body.index("STC(")


@pytest.mark.parametrize("op,tak", VARIANTS, ids=IDS)
def test_projector_default_is_the_complex128_form(op, tak):
    src = hip.projector_source(op, KSHAPE, tak)
    assert src == hip.projector_source(op, KSHAPE, tak, ctype="complex128")
    assert src == hip.projector_source(op, KSHAPE, tak,
                                       ctype=torch.complex128)
    assert not re.search(r"\bfloat", src)
    assert "widen" not in src
    params = _params(src, f"proj_{op}")
    assert all(p.startswith(("double* __restrict__ ",
                             "const double* __restrict__ "))
               for p in params)
    assert src != hip.projector_source(op, KSHAPE, tak, ctype="complex64")


def test_spectra_bin_c64_source():
    src = hip.spectra_bin_source(700, ctype="complex64")
    assert "#define NBINS 700\n" in src
    assert _params(src, "spectra_bin_c64") == [
        "const float2* __restrict__ fk", "const double* __restrict__ wbase",
        "const int* __restrict__ bidx", "double* __restrict__ hist", "int n"]
    assert "__shared__ double lh[NBINS];" in src
    assert "const float2 v = fk[i];" in src
    assert "const double re = (double)v.x;" in src
    assert "const double im = (double)v.y;" in src
    assert "wbase[i] * (re * re + im * im)" in src
    # the one float2 is the loaded mode; nothing else is single
    assert not re.search(r"\bfloat\b", src)
    assert len(re.findall(r"\bfloat2\b", src)) == 2


def test_spectra_bin_default_is_the_complex128_form():
    src = hip.spectra_bin_source(700)
    assert src == hip.spectra_bin_source(700, ctype="complex128")
    assert not re.search(r"\bfloat", src)
    assert _params(src, "spectra_bin")[0] == "const double* __restrict__ fk"
    assert "const double re = fk[2 * i];" in src
    c64 = hip.spectra_bin_source(700, ctype="complex64")
    # the two forms differ in the name, the pointer and the load alone
    changed = [ln for ln in difflib.unified_diff(
        src.splitlines(), c64.splitlines(), lineterm="", n=0)
        if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
    assert len(changed) == 9, changed


def test_unknown_storage_types_are_refused():
    for bad in ("float32", torch.float64, None, "complex32"):
        with pytest.raises(ValueError):
            hip.projector_source("vec_to_pol", KSHAPE, ctype=bad)
        with pytest.raises(ValueError):
            hip.spectra_bin_source(37, ctype=bad)


def test_source_generation_needs_no_native_module(monkeypatch):
    def no_ext():
        raise AssertionError("source generation touched the native module")
    monkeypatch.setattr(hip, "ext", no_ext)
    for op, tak in VARIANTS:
        assert hip.projector_source(op, KSHAPE, tak, ctype="complex64")
    assert hip.spectra_bin_source(37, ctype="complex64")


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_c64_sources_compile_for_gfx950(tmp_path):
    """Device-only cross-compilation of every complex64 source, to
    assembly: no scratch, and every load of a thread is issued before its
    first store (outputs are routinely views of the input)."""
    sources = {ident: hip.projector_source(op, KSHAPE, tak,
                                           ctype="complex64")
               for (op, tak), ident in zip(VARIANTS, IDS)}
    sources["spectra_bin_c64"] = hip.spectra_bin_source(
        700, ctype="complex64")
    procs = []
    for form, src in sources.items():
        path = tmp_path / f"{form}.hip"
        path.write_text(src)
        procs.append((form, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-include", "hip/hip_runtime.h",
             "-S", str(path), "-o", str(tmp_path / f"{form}.s")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for form, proc in procs:
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (form, out[-3000:])
        asm = (tmp_path / f"{form}.s").read_text()
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", asm), form
        if form == "spectra_bin_c64":
            continue
        code = asm[:asm.index("s_endpgm")]
        ops = re.findall(r"^\s*(global_(?:load|store)_\w+)", code, re.M)
        loads = [i for i, o in enumerate(ops) if "load" in o]
        stores = [i for i, o in enumerate(ops) if "store" in o]
        assert loads and stores and max(loads) < min(stores), (form, ops)
        # a mode is one 8-byte access either way
        data = [o for o in ops if o.endswith("dwordx2")]
        nstore = sum(WRITTEN[form.split("-")[0]].values())
        assert len(stores) == nstore, (form, ops)
        assert all(ops[i].endswith("dwordx2") for i in stores), (form, ops)
        assert len(data) >= nstore


# -- the CPU path: the torch expressions, never a kernel

def _raise(*args, **kwargs):
    raise AssertionError("the CPU path reached a fused kernel")


def test_float32_cpu_spectra_meet_the_end_to_end_bound(monkeypatch):
    for name in ("spectra_bin", "spectra_bin_c64", "projector_op",
                 "projector_op_c64", "tt_project_c64"):
        monkeypatch.setattr(hip, name, _raise, raising=False)
    got = run_spectra(np.float32, "cpu")
    assert_end_to_end(got)

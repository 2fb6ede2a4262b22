"""The fused Rayleigh mode kernel (backend/hip.py ``rayleigh_source``):
the source of every form, generated and inspected without a device or
the native module, and cross-compiled for gfx950 where hipcc is present.
"""

import itertools
import os
import re
import shutil
import subprocess

import pytest
import torch

from pystella_amd.backend import hip

GRID = (12, 10, 14)
FORMS = list(itertools.product(
    (False, True), (True, False), ("complex128", "complex64")))


def _kshape(is_real):
    return (12, 10, 8) if is_real else GRID


def _source(wkb, is_real, ctype, random=True):
    return hip.rayleigh_source(_kshape(is_real), GRID, wkb=wkb,
                               is_real=is_real, random=random, ctype=ctype)


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _ids(form):
    wkb, is_real, ctype = form
    return "-".join(("wkb" if wkb else "generate",
                     "r2c" if is_real else "c2c", ctype))


@pytest.fixture
def no_ext(monkeypatch):
    def raises():
        raise AssertionError("rayleigh_source touched the native module")
    monkeypatch.setattr(hip, "ext", raises)


@pytest.mark.parametrize("form", FORMS, ids=_ids)
def test_parameter_lists(form, no_ext):
    wkb, is_real, ctype = form
    src = _source(*form)
    ct = {"complex128": "double2", "complex64": "float2"}[ctype]
    kshape = _kshape(is_real)
    defines = dict(re.findall(r"^#define (\w+) (\S+)$", src, re.M))
    assert [defines[n] for n in ("NKX", "NKY", "NKZ")] == \
        [str(n) for n in kshape]
    assert [defines[n] for n in ("NX", "NY", "NZ")] == [str(n) for n in GRID]
    assert defines["WKB"] == str(int(wkb))
    assert defines["IS_REAL"] == str(int(is_real))
    assert defines["RANDOM"] == "1"
    assert "if (idx >= VOLK) return;" in src
    assert "__launch_bounds__(256)" in src
    params = _params(src, "rayleigh_modes")
    tables = [f"const int* __restrict__ {t}" for t in ("gxs", "gys", "gzs")]
    ints = ["const int seed_lo", "const int seed_hi", "const int draw"]
    if wkb:
        assert params == [
            f"{ct}* __restrict__ fk", f"{ct}* __restrict__ dfk",
            "const double* __restrict__ sqrt_power",
            "const double* __restrict__ omega"] + tables + ints + [
            "const double hubble"]
    else:
        assert params == [
            f"{ct}* __restrict__ fk",
            "const double* __restrict__ sqrt_power"] + tables + ints
        body = src[src.index("void rayleigh_modes"):]
        for name in ("dfk", "omega", "hubble"):
            assert not re.search(r"\b%s\b" % name, body), name
    # one store per output, a whole complex value each
    stores = re.findall(r"^\s*(\w+)\[idx\] = make_(\w+)\(", src, re.M)
    assert stores == [("fk", ct)] + ([("dfk", ct)] if wkb else [])
    # ten rounds written out; the high products are __umulhi
    assert src.count("PHILOX_ROUND(k0") == 10
    assert "__umulhi(0xD2511F53u, c0)" in src
    assert "__umulhi(0xCD9E8D57u, c2)" in src
    assert "sincospi(2.0 * u_phs" in src


def test_flags_select_the_code(no_ext):
    unit = _source(True, True, "complex128", random=False)
    assert "#define RANDOM 0" in unit
    assert unit.replace("#define RANDOM 0", "#define RANDOM 1") == \
        _source(True, True, "complex128")
    # the dtype objects name the same forms as their names
    assert _source(False, True, torch.complex64) == \
        _source(False, True, "complex64")
    assert _source(False, True, torch.complex128) == \
        _source(False, True, "complex128")


def test_unknown_forms_are_refused(no_ext):
    with pytest.raises(ValueError, match="ctype"):
        _source(False, True, "float64")
    with pytest.raises(ValueError, match="3-tuples"):
        hip.rayleigh_source((12, 10), GRID, wkb=False, is_real=True,
                            random=True, ctype="complex128")
    with pytest.raises(TypeError):
        hip.rayleigh_source((12, 10, 8), GRID, True, True, True,
                            "complex128")


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_sources_compile_for_gfx950(tmp_path, no_ext):
    """Device-only cross-compilation of every form, and of a unit-
    amplitude one, with the JIT's options."""
    forms = {_ids(f): _source(*f) for f in FORMS}
    forms["wkb-r2c-unit"] = _source(True, True, "complex128", random=False)
    procs = []
    for form, src in forms.items():
        path = tmp_path / f"{form}.hip"
        path.write_text(src)
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

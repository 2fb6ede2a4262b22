"""The generated HIP source of the fused register-ring kernels
(backend/hip.py JitLapStage, JitLapReduction) for float32 and float64
fields, produced and inspected without a device, and cross-compiled for
gfx950 where hipcc is present.

What is pinned: the per-site type follows the fields' dtype (arrays,
ring, Laplacian, k-preloads, temporaries), the reductions and the
device state stay float64, no bare double literal or double scalar
promotes the float32 per-site arithmetic, the float32 Laplacian is the
cancellation-safe difference form, and every launch path refuses
arrays of another dtype before anything is launched.
"""

import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend.hip import JitLapReduction, JitLapStage
from pystella_amd.sectors import get_rho_and_p
from tests.preheat_reference import potential

GRID = (72, 11, 80)
DX = (5 / 12, 5 / 11, 5 / 13)
DT = 1e-3
STATE_MAP = {"a": 0, "hubble": 4}
DTYPES = {"float32": torch.float32, "float64": torch.float64}


def _slabs(h):
    nx, ny, nz = GRID
    return ((0, h, 0, ny, 0, nz), (nx - h, nx, 0, ny, 0, nz),
            (h, nx - h, 0, h, 0, nz), (h, nx - h, ny - h, ny, 0, nz),
            (h, nx - h, h, ny - h, 0, h),
            (h, nx - h, h, ny - h, nz - h, nz))


@functools.lru_cache(maxsize=None)
def components(h):
    from pystella_amd.fusion import (
        FusedLaplacianReduction, StencilRKStepper)
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    st = StencilRKStepper(ps.LowStorageRK54, [sector], derivs,
                          halo_shape=h, rank_shape=GRID, dt=DT,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p)
    red = {store: FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=GRID, grid_size=gsize, store_lap=store)
        for store in (False, True)}
    return st, red


@functools.lru_cache(maxsize=None)
def stage_kernel(h, dtype, periodic, stage=1):
    """The device-loop form of one stage's kernel, source only."""
    st, _ = components(h)
    kern, = st._stepper.steps[stage].ring_kernels(
        GRID, DTYPES[dtype], state_map=STATE_MAP,
        periodic=(periodic,) * 3, compile=False)
    assert isinstance(kern, JitLapStage) and kern.key is None
    assert kern.dtype == DTYPES[dtype]
    return kern


@functools.lru_cache(maxsize=None)
def sources(h, dtype):
    """{form: (kernel name, source)} of every form built for (h, dtype):
    the plain, periodic and shell stage kernels, the host-loop stage
    kernel (scalars by value) and both lap-reductions."""
    st, red = components(h)
    out = {}
    for form, periodic in (("plain", False), ("periodic", True)):
        k = stage_kernel(h, dtype, periodic)
        out[form] = (k.source, "rk_stage_red1_f")
    k = stage_kernel(h, dtype, False)
    out["shell"] = (k.shell_source(_slabs(h)), "rk_stage_red1_f_shell")
    # the last stage: its k stores are elided
    k = stage_kernel(h, dtype, True, stage=4)
    out["periodic_last"] = (k.source, "rk_stage_red4_f")
    host, = st._stepper.steps[0].ring_kernels(
        GRID, DTYPES[dtype], compile=False)
    out["host"] = (host.source, "rk_stage_red0_f")
    for store in (False, True):
        k = red[store].lap_reduction_kernel(GRID, 2, DTYPES[dtype],
                                            compile=False)
        assert isinstance(k, JitLapReduction) and k.key is None
        assert k.dtype == DTYPES[dtype]
        out[f"lapred_store{int(store)}"] = (k.source, "lapred_map")
    return out


FORMS = ("plain", "periodic", "shell", "periodic_last", "host",
         "lapred_store0", "lapred_store1")


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src,
                  re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _strip_real_casts(text):
    """Remove every ``real(...)`` functional cast with its argument."""
    out, i = [], 0
    while True:
        j = text.find("real(", i)
        if j < 0 or (j and (text[j - 1].isalnum() or text[j - 1] == "_")):
            if j < 0:
                out.append(text[i:])
                return "".join(out)
            out.append(text[i:j + 5])
            i = j + 5
            continue
        out.append(text[i:j])
        depth, k = 1, j + 5
        while depth:
            depth += {"(": 1, ")": -1}.get(text[k], 0)
            k += 1
        i = k
        out.append("R")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("h", [2, 4])
def test_float32_source_honours_dtype(h, form):
    src, name = sources(h, "float32")[form]
    assert "using real = float;" in src
    params = _params(src, name)
    ptrs = [p for p in params if "*" in p]
    fields = [p for p in ptrs
              if p.split()[-1] not in ("partials", "state")]
    assert fields and all(p.startswith("real* __restrict__")
                          for p in fields), ptrs
    assert "double* __restrict__ partials" in ptrs
    if form not in ("host", "lapred_store0", "lapred_store1"):
        assert "const double* __restrict__ state" in ptrs
    # run-time scalars are passed as double and narrowed on use
    scalars = [p for p in params if "*" not in p
               and not p.startswith("const int")]
    assert all(p.startswith("double s_") for p in scalars), scalars
    # reductions stay float64
    assert "double acc[NRED];" in src
    assert "__shared__ double sd[TBZ * TBY];" in src
    # per-site storage is real
    assert "real ring[NF][2 * H + 1];" in src
    assert "real lapv[NF];" in src
    assert re.search(r"const real\* fp = f \+", src)
    assert not re.search(r"\bdouble\s+(ring|lapv|la)\b", src)
    assert not re.search(r"\bdouble\s*\*\s*(fp|cp)\b", src)
    assert not re.search(r"const double (pl_|rhs_|knew_|lapv_)", src)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("h", [2, 4])
def test_float32_per_site_arithmetic_is_not_promoted(h, form):
    """Outside the reducer lines (whose value is widened on purpose)
    and the declarations of double quantities, every floating literal
    and every run-time scalar of the kernel body sits inside a
    ``real(...)`` cast."""
    src, name = sources(h, "float32")[form]
    body = src[src.index("void " + name):]
    body = body[body.index(")\n{") + 2:body.index("__shared__ double sd")]
    checked = 0
    for line in body.splitlines():
        if "acc[" in line or "const double std_" in line:
            continue
        bare = _strip_real_casts(line)
        assert not re.search(r"(?<![\w.])\d+\.\d*(e[-+]?\d+)?(?![\w.])",
                             bare), line
        assert not re.search(r"(?<![\w.])\d+e[-+]?\d+", bare), line
        assert not re.search(r"\b(s_\w+|std_\w+|state\[|LAPC0)", bare), \
            line
        checked += 1
    assert checked > 10
    # the difference form: the centre value leaves every neighbour
    # before any coefficient is applied, and no c0*f0 term remains
    terms = [ln for ln in body.splitlines() if "la +=" in ln]
    assert len(terms) == h
    for ln in terms:
        assert ln.count("- f0)") == 6, ln
        assert "ring[fld][H] *" not in ln
    assert "real la = real(0.0);" in body
    assert "* LAPC0" not in body


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("h", [2, 4])
def test_float64_source_keeps_its_form(h, form):
    src, name = sources(h, "float64")[form]
    assert "using real = double;" in src
    ptrs = [p for p in _params(src, name) if "*" in p]
    assert all("double* __restrict__" in p for p in ptrs), ptrs
    assert "double la = ring[fld][H] * LAPC0;" in src
    assert "- f0)" not in src and "std_" not in src
    assert "double ring[NF][2 * H + 1];" in src


def test_reducers_take_the_scale_factor_in_double():
    """A scale factor narrowed to float32 is off by up to 6e-8 at every
    site alike; the reducers that feed the float64 Friedmann ODE read
    the double."""
    src, _ = sources(2, "float32")["plain"]
    red = [ln for ln in src.splitlines() if "acc[" in ln and "const double b"
           in ln]
    assert len(red) == 5
    assert sum("std_a" in ln for ln in red) == 4     # kinetic, gradient
    assert not any("st_a" in ln for ln in red)
    assert "const real st_a = real(std_a);" in src
    src, _ = sources(2, "float32")["lapred_store0"]
    red = [ln for ln in src.splitlines() if "const double b" in ln]
    assert sum(re.search(r"\(s_a\)", ln) is not None for ln in red) == 4
    assert not any("real(s_a)" in ln for ln in red)


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("h", [2, 4])
def test_float32_sources_compile_for_gfx950(h, tmp_path):
    """Device-only cross-compilation of every float32 form."""
    procs = []
    for form in FORMS:
        src, _ = sources(h, "float32")[form]
        path = tmp_path / f"{form}.hip"
        path.write_text(src)
        procs.append((form, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-Werror=implicit-float-conversion",
             "-include", "hip/hip_runtime.h",
             "-c", str(path), "-o", str(tmp_path / f"{form}.co")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for form, proc in procs:
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (form, out[-3000:])
        assert (tmp_path / f"{form}.co").stat().st_size > 0


# -- the dtype guard, on every launch path, with plain CPU tensors: the
# dtype is looked at before the device, and before anything is launched

def _env(h, dtypes):
    pad = tuple(n + 2 * h for n in GRID)
    env = {"f": torch.zeros((2,) + pad, dtype=dtypes["f"]),
           "f_next": torch.zeros((2,) + pad, dtype=dtypes["f_next"]),
           "dfdt": torch.zeros((2,) + pad, dtype=dtypes["dfdt"]),
           "f_tmp": torch.zeros((2,) + GRID, dtype=dtypes["f_tmp"]),
           "dfdt_tmp": torch.zeros((2,) + GRID, dtype=dtypes["dfdt_tmp"]),
           "state": torch.zeros(8, dtype=torch.float64),
           "dt": DT, "rk_a0": 0.0}
    return env


class _Compiled:
    """Stands in for a compiled kernel handle: the guard must fire
    before the handle is used."""


@pytest.mark.parametrize("bad", ["f", "f_next", "dfdt", "f_tmp",
                                 "dfdt_tmp"])
@pytest.mark.parametrize("kdtype", ["float32", "float64"])
def test_launch_paths_refuse_other_dtypes(kdtype, bad, monkeypatch):
    other = {"float32": torch.float64, "float64": torch.float32}[kdtype]
    dtypes = dict.fromkeys(("f", "f_next", "dfdt", "f_tmp", "dfdt_tmp"),
                           DTYPES[kdtype])
    dtypes[bad] = other
    env = _env(2, dtypes)
    kern = stage_kernel(2, kdtype, False)
    monkeypatch.setattr(kern, "key", _Compiled())
    partials = torch.zeros((5, 4), dtype=torch.float64)
    box = (0,) + GRID[:1] + (0,) + GRID[1:2] + (0,) + GRID[2:]
    calls = {
        "launch_box": lambda: kern.launch_box(env, box, partials, 0, 4),
        "launch_shell": lambda: kern.launch_shell(env, _slabs(2), partials,
                                                  0, 4),
        "launch_only": lambda: kern.launch_only(env),
        "__call__": lambda: kern(env),
    }
    for path, call in calls.items():
        with pytest.raises(TypeError, match=rf"argument {bad} has dtype "
                           rf"{re.escape(str(other))}"):
            call()


@pytest.mark.parametrize("kdtype", ["float32", "float64"])
def test_lap_reduction_refuses_other_dtypes(kdtype, monkeypatch):
    other = {"float32": torch.float64, "float64": torch.float32}[kdtype]
    _, red = components(2)
    kern = red[False].lap_reduction_kernel(GRID, 2, DTYPES[kdtype],
                                           compile=False)
    monkeypatch.setattr(kern, "key", _Compiled())
    pad = tuple(n + 4 for n in GRID)
    env = {"f": torch.zeros((2,) + pad, dtype=DTYPES[kdtype]),
           "dfdt": torch.zeros((2,) + pad, dtype=other), "a": 1.0}
    with pytest.raises(TypeError, match="argument dfdt has dtype"):
        kern(env)


def test_state_buffer_must_stay_float64(monkeypatch):
    kern = stage_kernel(2, "float32", False)
    monkeypatch.setattr(kern, "key", _Compiled())
    env = _env(2, dict.fromkeys(
        ("f", "f_next", "dfdt", "f_tmp", "dfdt_tmp"), torch.float32))
    env["state"] = env["state"].float()
    with pytest.raises(TypeError, match="argument state has dtype"):
        kern.launch_only(env)


def test_source_only_kernel_cannot_be_launched():
    kern = stage_kernel(2, "float32", False)
    env = _env(2, dict.fromkeys(
        ("f", "f_next", "dfdt", "f_tmp", "dfdt_tmp"), torch.float32))
    with pytest.raises(RuntimeError, match="compile=False"):
        kern.launch_only(env)


def test_drivers_refuse_mixed_field_dtypes():
    """The drivers infer the kernels' dtype from the field arrays; a
    mix is refused by name before any kernel is built."""
    from pystella_amd.fusion import _field_dtype
    st, red = components(2)
    smap = st._stepper.steps[0]
    env = _env(2, {"f": torch.float32, "f_next": torch.float32,
                   "dfdt": torch.float64, "f_tmp": torch.float32,
                   "dfdt_tmp": torch.float32})
    with pytest.raises(TypeError, match=r"dfdt: torch\.float64.*f: torch\.float32"):
        smap._env_dtype(env)
    env["dfdt"] = env["dfdt"].float()
    assert smap._env_dtype(env) == torch.float32
    assert _field_dtype({}, red[False].field_args) == torch.float64

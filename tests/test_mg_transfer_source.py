"""The fused multigrid transfer kernels (backend/hip.py
``mg_transfer_source``): the source of every form, generated and
inspected without a device and cross-compiled for gfx950 where hipcc is
present; and the CPU results of the four transfer operators, which never
reach those kernels.
"""

import itertools
import os
import re
import shutil
import subprocess

import pytest
import torch

from pystella_amd.backend import hip
from pystella_amd.multigrid.transfer import (
    CubicInterpolation, FullWeighting, Injection, LinearInterpolation)

# name -> (kind, coefficients as mg_transfer_source takes them, halo,
#          stores per thread and loop trip)
SETS = {
    "full_weighting": ("restrict", FullWeighting(1).coefs, 1, 1),
    "full_weighting_h2": ("restrict", FullWeighting(2).coefs, 2, 1),
    "injection": ("restrict", Injection(1).coefs, 1, 1),
    "linear": ("interpolate", (LinearInterpolation(1).even,
                               LinearInterpolation(1).odd), 1, 4),
    "cubic": ("interpolate", (CubicInterpolation(2).even,
                              CubicInterpolation(2).odd), 2, 4),
}
DTYPES = {"float32": "float", "float64": "double"}
FORMS = list(itertools.product(SETS, DTYPES, (False, True)))


def _name(kind, correct):
    return f"mg_{kind}" + ("_correct" if correct else "")


def _source(form, dtype, correct):
    kind, coefs, halo, _ = SETS[form]
    return hip.mg_transfer_source(kind, coefs, halo, dtype, correct)


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("form,dtype,correct", FORMS)
def test_source_types_stores_and_run_time_extents(form, dtype, correct):
    kind, coefs, halo, nstores = SETS[form]
    src = _source(form, dtype, correct)
    assert f"using real = {DTYPES[dtype]};" in src
    assert f"#define H {halo}\n" in src
    params = _params(src, _name(kind, correct))
    # the arrays are real*, the input const; the extents are run-time ints
    ins, outs = ("f1", "f2") if kind == "restrict" else ("f2", "f1")
    assert sorted(params[:2]) == sorted([
        f"const real* __restrict__ {ins}", f"real* __restrict__ {outs}"])
    assert params[2:] == ["const int n2x", "const int n2y", "const int n2z",
                          "const int nouter"]
    for n in ("NX", "NY", "NZ"):
        assert f"#define {n}" not in src
    # every value that is summed is a double; nothing is a float but real
    assert "float" not in src.replace(f"using real = {DTYPES[dtype]};", "")
    values = re.findall(r"const (\w+) (?:[xyzs]|cz)[\d_]* =", src)
    assert values and set(values) == {"double"}
    # every load is widened on the spot
    loads = re.findall(r"(\(double\))?(r\d+_\d+|%s)\[" % outs, src)
    loads = [ld for ld in loads if ld[1] != outs]
    assert loads and all(cast for cast, _ in loads)
    # one store per output site, each one rounding of a double
    stores = re.findall(r"^\s*%s\[([^\]]+)\] = \(real\)(.*);$" % outs, src,
                        re.M)
    assert len(stores) == nstores
    assert len({at for at, _ in stores}) == nstores
    # correct reads each output site exactly once, on its store's line
    reads = re.findall(r"\(double\)%s\[([^\]]+)\]" % outs, src)
    if correct:
        assert reads == [at for at, _ in stores]
        sign = "-" if kind == "restrict" else "+"
        for at, val in stores:
            assert re.fullmatch(
                r"\(\(double\)%s\[%s\] \%s s\d*\)" % (outs, re.escape(at),
                                                     sign), val), val
    else:
        assert reads == []
        assert all(re.fullmatch(r"s\d*", val) for _, val in stores)
    assert src.count(f"{outs}[") == nstores * (2 if correct else 1)
    # linear offsets are long
    assert re.search(r"const long sy1 = .*sx1 = ", src)
    assert "const long d = " in src and "const long ntiles" in src
    assert "for (long t = blockIdx.x; t < ntiles; t += gridDim.x)" in src


@pytest.mark.parametrize("form", SETS)
def test_coefficients_are_baked_in_as_double_literals(form):
    kind, coefs, halo, _ = SETS[form]
    src = _source(form, "float32", False)
    sets = [coefs] if kind == "restrict" else list(coefs)
    for cs in sets:
        for c in cs.values():
            assert f"{float(c)!r} * " in src
    assert not re.search(r"\d\.\d+f\b", src)


def test_term_counts_are_separable():
    """3+3+3, not 27: nine x sums of three loads, three y sums, one z."""
    src = _source("full_weighting", "float64", False)
    assert len(re.findall(r"\(double\)r\d_\d\[", src)) == 27   # loads
    assert len(re.findall(r"const double x\d_\d = ", src)) == 9
    assert len(re.findall(r"const double y\d = ", src)) == 3
    assert len(re.findall(r"const double s = ", src)) == 1
    src = _source("injection", "float64", False)
    assert len(re.findall(r"\(double\)r\d_\d\[", src)) == 1
    # linear prolongation: the pair of fine sites reads two coarse sites
    # per axis, 8 loads for this thread's 4 fine sites
    src = _source("linear", "float64", False)
    assert len(re.findall(r"\(double\)r\d_\d\[", src)) == 8
    src = _source("cubic", "float64", False)
    assert len(re.findall(r"\(double\)r\d_\d\[", src)) == 64


def test_lane_parity_selects_coefficients_without_a_branch():
    want = {"linear": ["pk ? 0.5 : 1.0", "pk ? 0.5 : 0.0"],
            "cubic": ["pk ? -0.0625 : 0.0", "pk ? 0.5625 : 1.0",
                      "pk ? 0.5625 : 0.0", "pk ? -0.0625 : 0.0"]}
    for form, selects in want.items():
        src = _source(form, "float32", True)
        assert "const int pk = lz & 1;" in src
        assert re.findall(r"const double cz\d = (.*);", src) == selects
        # every lane loads the whole union of both parities' sites
        n = len(selects)
        rows = re.findall(r"const double z\d_\d = (.*);", src)
        assert len(rows) == n * n
        for row in rows:
            assert re.findall(r"cz(\d) \* \(double\)r", row) == \
                [str(c) for c in range(n)]
        assert src.count("pk") == 1 + n
        assert "if (pk" not in src and "if (lz &" not in src


def test_offsets_must_fit_the_halo():
    with pytest.raises(ValueError):
        hip.mg_transfer_source("restrict", {-2: .5, 2: .5}, 1, "float64")
    cubic = CubicInterpolation(2)
    with pytest.raises(ValueError):
        hip.mg_transfer_source("interpolate", (cubic.even, cubic.odd), 1,
                               "float64")
    with pytest.raises(ValueError):
        hip.mg_transfer_source("smooth", {0: 1.}, 1, "float64")
    with pytest.raises(TypeError):
        hip.mg_transfer_source("restrict", {0: 1.}, 1, "float16")
    with pytest.raises(ValueError):
        hip.mg_transfer_source("restrict", {0: float("nan")}, 1, "float64")


def test_interpolation_offsets_follow_the_axis_rule():
    for op in (LinearInterpolation(1), CubicInterpolation(2)):
        assert hip.mg_interpolation_offsets(op.even, op.odd) == (
            op._axis_coefs(0), op._axis_coefs(1))


def test_source_generation_needs_no_native_module(monkeypatch):
    def no_ext():
        raise AssertionError("mg_transfer_source touched the native module")
    monkeypatch.setattr(hip, "ext", no_ext)
    for form, dtype, correct in FORMS:
        assert _source(form, dtype, correct)
    # one operator object, one source per dtype: nothing about a level
    assert _source("linear", torch.float32, True) == \
        _source("linear", "float32", True)


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)

COMPILE_SET = [
    ("full_weighting", "float32", False),
    ("full_weighting", "float64", True),
    ("full_weighting_h2", "float32", True),
    ("injection", "float64", False),
    ("linear", "float32", True),
    ("linear", "float64", False),
    ("cubic", "float32", False),
    ("cubic", "float64", True),
]


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_sources_compile_for_gfx950(tmp_path):
    """Device-only cross-compilation of a representative set."""
    procs = []
    for form, dtype, correct in COMPILE_SET:
        stem = f"{form}_{dtype}_{int(correct)}"
        path = tmp_path / f"{stem}.hip"
        path.write_text(_source(form, dtype, correct))
        procs.append((stem, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-include", "hip/hip_runtime.h",
             "-c", str(path), "-o", str(tmp_path / f"{stem}.co")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for stem, proc in procs:
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (stem, out[-3000:])
        assert (tmp_path / f"{stem}.co").stat().st_size > 0


# -- the CPU path: today's torch chain, never the fused kernels

def _cpu_results():
    gen = torch.Generator().manual_seed(15)
    out = []
    for h, dtype in ((1, torch.float64), (2, torch.float32)):
        n2 = (3, 4, 5)
        fine = (2,) + tuple(2 * n + 2 * h for n in n2)
        coarse = (2,) + tuple(n + 2 * h for n in n2)
        ops = [FullWeighting, Injection, LinearInterpolation]
        if h >= 2:
            ops.append(CubicInterpolation)
        for make in ops:
            for correct in (False, True):
                f1 = torch.rand(fine, dtype=dtype, generator=gen)
                f2 = torch.rand(coarse, dtype=dtype, generator=gen)
                ret = make(halo_shape=h, correct=correct)(f1=f1, f2=f2)
                assert ret is (f2 if make in (FullWeighting, Injection)
                               else f1)
                out.append(ret)
    return out


def _raise(*args, **kwargs):
    raise AssertionError("the CPU path reached a fused transfer kernel")


def test_cpu_results_unchanged_without_the_kernels(monkeypatch):
    want = _cpu_results()
    monkeypatch.setattr(hip, "mg_restrict", _raise)
    monkeypatch.setattr(hip, "mg_interpolate", _raise)
    got = _cpu_results()
    assert len(got) == len(want) == 14
    for g, w in zip(got, want):
        assert w.abs().max() > 0
        assert torch.equal(g, w)

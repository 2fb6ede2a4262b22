"""The fused k-space kernels of SpectralCollocator and
SpectralPoissonSolver (backend/hip.py ``kspace_source``): the source of
every form, generated and inspected without a device and cross-compiled
for gfx950 where hipcc is present; and the CPU results of both classes,
which never reach those kernels.
"""

import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.derivs import SecondCenteredDifference
from pystella_amd.fourier import DFT

GRID = (12, 10, 14)
KSHAPE = (12, 10, 8)
LENGTHS = (5., 3., 7.)
OUTS = ("pdx", "pdy", "pdz", "lap")
MASKS = [m for r in range(1, 5) for m in itertools.combinations(OUTS, r)]
GRAD = ("pdx", "pdy", "pdz")


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _header(src):
    return [ln for ln in src.splitlines() if ln.startswith("#define")]


def test_there_are_fifteen_masks():
    assert len(MASKS) == 15 and len(set(MASKS)) == 15


@pytest.mark.parametrize("mask", MASKS, ids="+".join)
def test_derivs_source_declares_exactly_the_requested_outputs(mask):
    src = hip.kspace_source("derivs", KSHAPE, outs=mask)
    assert _header(src)[:3] == ["#define NKX 12", "#define NKY 10",
                                "#define NKZ 8"]
    assert "#define VOLK ((long)NKX * NKY * NKZ)" in src
    assert "if (idx >= VOLK) return;" in src
    params = _params(src, "kspace_derivs")
    assert params[0] == "const double2* __restrict__ fk"
    written = [p.split()[-1] for p in params if p.startswith("double2*")]
    assert written == [o for o in OUTS if o in mask]
    tables = [p.split()[-1] for p in params if p.startswith("const double*")]
    want = [f"k1{ax}" for ax in "xyz" if f"pd{ax}" in mask]
    want += ["k2x", "k2y", "k2z"] if "lap" in mask else []
    assert tables == want
    assert params[-1] == "const double inv_n"
    # every store is to a requested output, one 16-byte store each
    stores = re.findall(r"^\s*(\w+)\[idx\] = make_double2", src, re.M)
    assert stores == written
    # the order of the mask does not matter
    assert src == hip.kspace_source("derivs", KSHAPE, outs=mask[::-1])


@pytest.mark.parametrize("mu", [0, 1, 2])
@pytest.mark.parametrize("accumulate", [False, True])
def test_div_accum_source(mu, accumulate):
    src = hip.kspace_source("div_accum", KSHAPE, mu=mu,
                            accumulate=accumulate)
    params = _params(src, "kspace_div_accum")
    assert params == ["const double2* __restrict__ fk",
                      "double2* __restrict__ div_k",
                      "const double* __restrict__ k1", "const double inv_n"]
    assert f"k1[{('ii', 'jj', 'kk')[mu]}]" in src
    assert ("= div_k[idx];" in src) == accumulate


def test_poisson_source_takes_the_mass_at_run_time():
    src = hip.kspace_source("poisson", KSHAPE)
    params = _params(src, "kspace_poisson")
    assert params[-2:] == ["const double inv_n", "const double m_squared"]
    # sol may be rhok: neither is declared restrict
    assert params[:2] == ["const double2* rhok", "double2* sol"]
    assert "(mk2 < 0.0)" in src


def test_products_are_rounded_before_they_are_added():
    """The JIT's -ffp-contract=fast would fuse these into multiply-adds,
    which are not the torch chain's operations."""
    src = hip.kspace_source("derivs", KSHAPE, outs=("lap",))
    assert ("-((rounded(kx * kx) + rounded(ky * ky))\n"
            "                         + rounded(kz * kz));") in src
    src = hip.kspace_source("div_accum", KSHAPE, mu=0, accumulate=True)
    assert "d.x + rounded(term.x), d.y + rounded(term.y)" in src


def test_unknown_forms_are_refused():
    with pytest.raises(ValueError):
        hip.kspace_source("curl", KSHAPE)
    with pytest.raises(ValueError):
        hip.kspace_source("derivs", KSHAPE, outs=())
    with pytest.raises(ValueError):
        hip.kspace_source("derivs", KSHAPE, outs=("pdw",))
    with pytest.raises(ValueError):
        hip.kspace_source("div_accum", KSHAPE, mu=3, accumulate=False)
    with pytest.raises(TypeError):
        hip.kspace_source("poisson", KSHAPE, accumulate=True)


def test_source_generation_needs_no_native_module(monkeypatch):
    def no_ext():
        raise AssertionError("kspace_source touched the native module")
    monkeypatch.setattr(hip, "ext", no_ext)
    for mask in MASKS:
        assert hip.kspace_source("derivs", KSHAPE, outs=mask)
    assert hip.kspace_source("div_accum", KSHAPE, mu=1, accumulate=True)
    assert hip.kspace_source("poisson", KSHAPE)


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)

COMPILE_SET = {
    "lap": ("derivs", {"outs": ("lap",)}),
    "pdz": ("derivs", {"outs": ("pdz",)}),
    "grad": ("derivs", {"outs": GRAD}),
    "grad_lap": ("derivs", {"outs": GRAD + ("lap",)}),
    "div_store": ("div_accum", {"mu": 0, "accumulate": False}),
    "div_accumulate": ("div_accum", {"mu": 2, "accumulate": True}),
    "poisson": ("poisson", {}),
}


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_sources_compile_for_gfx950(tmp_path):
    """Device-only cross-compilation of a representative set."""
    procs = []
    for form, (op, flags) in COMPILE_SET.items():
        path = tmp_path / f"{form}.hip"
        path.write_text(hip.kspace_source(op, KSHAPE, **flags))
        procs.append((form, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-include", "hip/hip_runtime.h",
             "-c", str(path), "-o", str(tmp_path / f"{form}.co")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for form, proc in procs:
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (form, out[-3000:])
        assert (tmp_path / f"{form}.co").stat().st_size > 0


# -- the CPU path: today's torch chain, never the fused kernels

def _collocator_results():
    h = 1
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    dk = tuple(2 * np.pi / li for li in LENGTHS)
    fft = DFT(decomp, grid_shape=GRID, dtype=np.float64)
    coll = ps.SpectralCollocator(fft, dk)
    pad = tuple(n + 2 * h for n in GRID)
    gen = torch.Generator().manual_seed(11)
    fx = torch.rand((2,) + pad, dtype=torch.float64, generator=gen)
    lap = torch.zeros((2,) + pad, dtype=torch.float64)
    grd = torch.zeros((2, 3) + GRID, dtype=torch.float64)
    coll(fx=fx, lap=lap, grd=grd)
    vec = torch.rand((2, 3) + pad, dtype=torch.float64, generator=gen)
    div = torch.zeros((2,) + GRID, dtype=torch.float64)
    coll.divergence(vec=vec, div=div)
    return lap, grd, div


def _poisson_results():
    h = 1
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    dk = tuple(2 * np.pi / li for li in LENGTHS)
    dx = tuple(li / n for li, n in zip(LENGTHS, GRID))
    fft = DFT(decomp, grid_shape=GRID, dtype=np.float64)
    solver = ps.SpectralPoissonSolver(
        fft, dk, dx, SecondCenteredDifference(h).get_eigenvalues)
    pad = tuple(n + 2 * h for n in GRID)
    gen = torch.Generator().manual_seed(12)
    rho = torch.rand(GRID, dtype=torch.float64, generator=gen)
    out = []
    for m2 in (0, 1.7):
        fx = torch.zeros(pad, dtype=torch.float64)
        solver(fx=fx, rho=rho, m_squared=m2)
        out.append(fx)
    return out


def _raise(*args, **kwargs):
    raise AssertionError("the CPU path reached a fused k-space kernel")


@pytest.mark.parametrize("results", [_collocator_results, _poisson_results])
def test_cpu_results_unchanged_without_the_kernels(results, monkeypatch):
    want = results()
    for name in ("kspace_derivs", "kspace_div_accum", "kspace_poisson"):
        monkeypatch.setattr(hip, name, _raise)
    got = results()
    for g, w in zip(got, want):
        assert w.abs().max() > 0
        assert torch.equal(g, w)

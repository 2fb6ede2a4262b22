"""CPU side of the float32 stage-kernel tests.  No GPU needed.

* The float32 numpy emulation (tests/preheat_emulation_fp32.py) stays
  within a quarter of every tolerance that tests/test_stage_fp32.py
  holds the float32 kernels to, for every halo order: the tolerances
  are tied to the float64 reference and to float32 rounding, not to
  what a kernel happens to give.
* The plain-form float32 Laplacian leaks the field's mean and misses
  the cancellation bounds by orders of magnitude; the difference form
  meets them (the same bounds the GPU test applies to the kernels).
* The torch-CPU oracle path of StencilRKStepper / FusedLaplacianReduction
  accepts float32 tensors and agrees with the emulation.
"""

import functools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.sectors import get_rho_and_p
from tests.preheat_emulation_fp32 import (
    TOL_FP32, deviations, laplacian_fp32, preheat_emulation_fp32,
    zero_mean_data)
from tests.preheat_reference import (
    MPL, initial_data, periodic_laplacian, potential, preheat_reference)

GRID = (72, 11, 80)
DX = (5 / 12, 5 / 11, 5 / 13)
DT = 1e-3
STEPS = 2


@functools.lru_cache(maxsize=None)
def reference(h, steps=STEPS):
    f0, df0 = zero_mean_data(GRID)
    return preheat_reference(f0, df0, DX, DT, steps, h)


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_emulation_within_quarter_of_tolerances(h, form="difference"):
    f0, df0 = zero_mean_data(GRID)
    emu = preheat_emulation_fp32(f0, df0, DX, DT, STEPS, h, form)
    dev = deviations(emu, reference(h), STEPS)
    print(f"h={h} {form}: " + ", ".join(
        f"{k} {v:.2e}" for k, v in dev.items()))
    for key, tol in TOL_FP32.items():
        assert dev[key] <= tol / 4, (key, dev[key], tol)


@pytest.mark.parametrize("h", [2, 4])
def test_difference_form_cancels_the_mean(h):
    """float32(0.193 + 1e-6 randn): the Laplacian's whole signal is
    2e-4.  Bound 1.5e-10 as for the kernels' stored Laplacian."""
    rng = np.random.default_rng(1)
    u = (0.193 + 1e-6 * rng.standard_normal((2,) + GRID)).astype(
        np.float32)
    want = periodic_laplacian(u.astype(np.float64), h, DX)
    err = {form: np.abs(laplacian_fp32(u, h, DX, form) - want).max()
           for form in ("plain", "difference")}
    print(f"h={h}: max|lap| {np.abs(want).max():.2e}, " + ", ".join(
        f"{k} {v:.2e}" for k, v in err.items()))
    assert err["difference"] <= 1.5e-10 / 2
    assert err["plain"] > 1e-6


@pytest.mark.parametrize("h", [2, 4])
def test_difference_form_full_loop_on_preheating_data(h):
    """Two RK54 steps from the inflaton-mean initial data: the bounds of
    the kernels' cancellation test, which the plain form misses."""
    f0, df0 = (x.astype(np.float32) for x in initial_data(GRID))
    ref = preheat_reference(f0, df0, DX, DT, STEPS, h)
    dev = {form: deviations(
        preheat_emulation_fp32(f0, df0, DX, DT, STEPS, h, form), ref,
        STEPS) for form in ("plain", "difference")}
    for form, d in dev.items():
        print(f"h={h} {form}: " + ", ".join(
            f"{k} {v:.2e}" for k, v in d.items()))
    d = dev["difference"]
    assert d["E"] <= 1.2e-8 / 2 and d["P"] <= 1.2e-8 / 2
    assert d["adot"] <= 5e-9 / 2 and d["a"] <= 5e-12 / 2
    assert dev["plain"]["E"] > 1.2e-8 * 10


def cpu_host_loop(f0, df0, h, steps, dtype):
    """StencilRKStepper + FusedLaplacianReduction + Expansion.step on
    CPU tensors of ``dtype`` (the torch oracle path)."""
    from pystella_amd.fusion import (
        FusedLaplacianReduction, StencilRKStepper)
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    pad = tuple(n + 2 * h for n in GRID)
    cut = (slice(None),) + (slice(h, -h),) * 3
    f = torch.zeros((2,) + pad, dtype=dtype)
    dfdt = torch.zeros_like(f)
    f[cut] = torch.as_tensor(f0).to(dtype)
    dfdt[cut] = torch.as_tensor(df0).to(dtype)
    st = StencilRKStepper(ps.LowStorageRK54, [sector], derivs,
                          halo_shape=h, rank_shape=GRID, dt=DT,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=GRID, grid_size=gsize, store_lap=False)
    e0 = red(f=f, dfdt=dfdt, a=np.ones(1))
    energies = {0: (float(np.asarray(e0["total"]).reshape(-1)[0]),
                    float(np.asarray(e0["pressure"]).reshape(-1)[0]))}
    ex = ps.Expansion(e0["total"], ps.LowStorageRK54, mpl=MPL)
    arrays = {"f": f, "dfdt": dfdt, "f_next": torch.zeros_like(f)}
    decomp.share_halos(arrays["f"])
    for n in range(steps):
        for s in range(st.num_stages):
            e_in = st(s, a=ex.a, hubble=ex.hubble, **arrays)
            arrays["f"], arrays["f_next"] = arrays["f_next"], arrays["f"]
            decomp.share_halos(arrays["f"])
            ex.step(s, e_in["total"], e_in["pressure"], DT)
            if s == st.num_stages - 1:
                energies[5 * n + 4] = (
                    float(np.asarray(e_in["total"]).reshape(-1)[0]),
                    float(np.asarray(e_in["pressure"]).reshape(-1)[0]))
    for name in ("f", "dfdt", "f_next"):
        assert arrays[name].dtype == dtype
    for t in st.tmp_arrays.values():
        assert t.dtype == dtype
    return (arrays["f"][cut].numpy(), arrays["dfdt"][cut].numpy(),
            float(ex.a[0]), float(ex.adot[0]), energies)


@pytest.mark.parametrize("h", [2, 4])
def test_cpu_oracle_accepts_float32(h):
    """One RK54 step of the host loop on float32 CPU tensors against
    the emulation, at the kernels' tolerances."""
    f0, df0 = zero_mean_data(GRID)
    emu = preheat_emulation_fp32(f0, df0, DX, DT, 1, h)
    got = cpu_host_loop(f0, df0, h, 1, torch.float32)
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    dev = deviations(got, emu, 1)
    print(f"h={h}: " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for key, tol in TOL_FP32.items():
        assert dev[key] <= tol, (key, dev[key], tol)

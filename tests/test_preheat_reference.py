"""Pins the independent numpy reference (tests/preheat_reference.py)
against the CPU host loop for every halo order, and checks the
PYSTELLA_TILE validation of JitLapStage.pick_tile.  No GPU needed.
"""

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.sectors import get_rho_and_p
from tests.preheat_reference import (
    MPL, fd_reference, initial_data, potential, preheat_reference)

GRID = (72, 11, 80)
DX = (5 / 12, 5 / 11, 5 / 13)
DT = 1e-3
STEPS = 2


def cpu_host_loop(f0, df0, dx, dt, steps, h):
    """StencilRKStepper + FusedLaplacianReduction + Expansion.step on
    the CPU (the torch oracle path of every fused kernel)."""
    from pystella_amd.fusion import FusedLaplacianReduction, StencilRKStepper
    grid = f0.shape[1:]
    gsize = float(np.prod(grid))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=grid)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, dx, rank_shape=grid)
    pad = tuple(n + 2 * h for n in grid)
    cut = (slice(None),) + (slice(h, -h),) * 3
    f = torch.zeros((2,) + pad, dtype=torch.float64)
    dfdt = torch.zeros_like(f)
    f[cut] = torch.as_tensor(f0)
    dfdt[cut] = torch.as_tensor(df0)

    st = StencilRKStepper(ps.LowStorageRK54, [sector], derivs,
                          halo_shape=h, rank_shape=grid, dt=dt,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=grid, grid_size=gsize, store_lap=False)
    e0 = red(f=f, dfdt=dfdt, a=np.ones(1))
    ex = ps.Expansion(e0["total"], ps.LowStorageRK54, mpl=MPL)
    arrays = {"f": f, "dfdt": dfdt, "f_next": torch.zeros_like(f)}
    decomp.share_halos(arrays["f"])
    for _ in range(steps):
        for s in range(st.num_stages):
            e_in = st(s, a=ex.a, hubble=ex.hubble, **arrays)
            arrays["f"], arrays["f_next"] = arrays["f_next"], arrays["f"]
            decomp.share_halos(arrays["f"])
            ex.step(s, e_in["total"], e_in["pressure"], dt)
    return (arrays["f"][cut].numpy(), arrays["dfdt"][cut].numpy(),
            float(ex.a[0]), float(ex.adot[0]))


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_reference_matches_cpu_host_loop(h):
    f0, df0 = initial_data(GRID)
    fr, dfr, ar, adr, energies = preheat_reference(
        f0, df0, DX, DT, STEPS, h)
    fc, dfc, ac, adc = cpu_host_loop(f0, df0, DX, DT, STEPS, h)
    assert len(energies) == 5 * STEPS + 1
    errs = {"f": np.abs(fc - fr).max(), "dfdt": np.abs(dfc - dfr).max(),
            "a": abs(ac - ar) / abs(ar), "adot": abs(adc - adr) / abs(adr)}
    print(f"h={h}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["f"] < 1e-14, errs
    assert errs["dfdt"] < 1e-14, errs
    assert errs["a"] < 1e-14, errs
    assert errs["adot"] < 1e-14, errs


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_fd_reference_differentiates_polynomials(h):
    """The literal coefficient tables are right: the order-2h centred
    first difference is exact (to rounding) on polynomials up to degree
    2h and the second difference up to degree 2h+1, so a mistyped
    coefficient shows up far above rounding."""
    n = (9, 8, 7)
    dx = (0.1, 0.11, 0.12)
    x, y, z = np.meshgrid(
        *[d * (np.arange(-h, m + h) - 2.5) for d, m in zip(dx, n)],
        indexing="ij")
    cut = (slice(h, -h),) * 3
    xi, yi, zi = x[cut], y[cut], z[cut]

    p = 2 * h
    _, pdx, pdy, pdz = fd_reference(
        x**p - 2 * y**p + 3 * z**p + x * y * z, h, dx)
    assert np.abs(pdx - (p * xi**(p - 1) + yi * zi)).max() < 1e-11
    assert np.abs(pdy - (-2 * p * yi**(p - 1) + xi * zi)).max() < 1e-11
    assert np.abs(pdz - (3 * p * zi**(p - 1) + xi * yi)).max() < 1e-11

    q = 2 * h + 1
    lap, _, _, _ = fd_reference(x**q - 2 * y**q + 3 * z**p, h, dx)
    want = (q * (q - 1) * xi**(q - 2) - 2 * q * (q - 1) * yi**(q - 2)
            + 3 * p * (p - 1) * zi**(p - 2))
    assert np.abs(lap - want).max() < 1e-9


@pytest.mark.parametrize("value", ["64,8", "64,x,8", "64,0,8", "64,-2,16",
                                   "64;4;32", "64,4,32,1"])
def test_pick_tile_rejects_malformed(value, monkeypatch):
    from pystella_amd.backend.hip import JitLapStage
    monkeypatch.setenv("PYSTELLA_TILE", value)
    with pytest.raises(ValueError, match="PYSTELLA_TILE"):
        JitLapStage.pick_tile((64, 64, 64))


def test_pick_tile_rejects_partial_wavefront(monkeypatch):
    from pystella_amd.backend.hip import JitLapStage
    monkeypatch.setenv("PYSTELLA_TILE", "32,3,8")
    with pytest.raises(ValueError, match="multiple of"):
        JitLapStage.pick_tile((64, 64, 64))
    # whole wavefronts, but the reduction tree needs a power of two
    for value in ("64,3,16", "64,32,16"):
        monkeypatch.setenv("PYSTELLA_TILE", value)
        with pytest.raises(ValueError, match="power of two"):
            JitLapStage.pick_tile((64, 64, 64))
    monkeypatch.setenv("PYSTELLA_TILE", "32,2,8")
    assert JitLapStage.pick_tile((64, 64, 64)) == (32, 2, 8)
    monkeypatch.delenv("PYSTELLA_TILE")
    assert JitLapStage.pick_tile((64, 64, 64)) in JitLapStage.TILE_CANDIDATES

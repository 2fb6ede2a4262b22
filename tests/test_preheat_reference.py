"""Pins the independent numpy reference (tests/preheat_reference.py)
against the CPU host loop for every halo order, and checks the
PYSTELLA_TILE validation of JitLapStage.pick_tile.  Its scalar +
tensor-perturbation form (gw_reference) is pinned the same way, also
for the split tensor families and the other 2N tableaus the GPU matrix
runs, and shown to be sensitive to the mistakes that matrix is there
to catch.  No GPU needed.
"""

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.sectors import get_rho_and_p
from tests.preheat_reference import (
    MPL, fd_reference, gw_reference, initial_data, initial_tensor_data,
    potential, preheat_reference)

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


def gw_tolerances():
    """The absolute tolerances of the GPU matrix
    (tests/test_stage_gw_variants.py) for the tensor arrays: the
    relative allowance tests/test_stage_variants.py gives ``f``
    (1e-12 / max|f| ~ 5e-12) and ``dfdt`` (1e-10 / max|dfdt| ~ 7e-10),
    scaled to max|hij| ~ 4.7e-3 and max|dhijdt| ~ 5e-3 of the
    reference."""
    return {"hij": 2.5e-14, "dhijdt": 3.5e-12}


def cpu_gw_host_loop(f0, df0, h0, dh0, dx, dt, steps, h,
                     Stepper=ps.LowStorageRK54, split=False):
    """The scalar + tensor host loop on the CPU: StencilRKStepper with
    inlined gradients and fused reducers, FusedLaplacianReduction for
    the seed energy, Expansion.step.  ``split``: two three-component
    tensor families that are views of one six-component parent array,
    as bench.py --gws-split builds them."""
    from pystella_amd.fusion import FusedLaplacianReduction, StencilRKStepper
    grid = f0.shape[1:]
    gsize = float(np.prod(grid))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=grid)
    sector = ps.ScalarSector(2, potential=potential)
    if split:
        tensors = [
            ps.TensorPerturbationSector(
                [sector], components=(0, 1, 2), name="hij_a"),
            ps.TensorPerturbationSector(
                [sector], components=(3, 4, 5), name="hij_b")]
    else:
        tensors = [ps.TensorPerturbationSector([sector])]
    derivs = ps.FiniteDifferencer(decomp, h, dx, rank_shape=grid)
    pad = tuple(n + 2 * h for n in grid)
    cut = (slice(None),) + (slice(h, -h),) * 3

    def padded(x):
        out = torch.zeros(x.shape[:1] + pad, dtype=torch.float64)
        out[cut] = torch.as_tensor(x)
        return out

    f, dfdt, hij, dhijdt = (padded(x) for x in (f0, df0, h0, dh0))
    hij_next = torch.zeros_like(hij)
    arrays = {"f": f, "dfdt": dfdt, "f_next": torch.zeros_like(f)}
    if split:
        arrays.update({
            "hij_a": hij[0:3], "hij_b": hij[3:6],
            "hij_a_next": hij_next[0:3], "hij_b_next": hij_next[3:6],
            "dhij_adt": dhijdt[0:3], "dhij_bdt": dhijdt[3:6]})
    else:
        arrays.update({"hij": hij, "hij_next": hij_next, "dhijdt": dhijdt})

    st = StencilRKStepper(Stepper, [sector] + tensors, derivs,
                          halo_shape=h, rank_shape=grid, dt=dt,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p, inline_grad=True)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=grid, grid_size=gsize, store_lap=False)
    e0 = red(f=f, dfdt=dfdt, a=np.ones(1))
    ex = ps.Expansion(e0["total"], Stepper, mpl=MPL)
    for name in st.pingpong:
        decomp.share_halos(arrays[name])
    for _ in range(steps):
        for s in range(st.num_stages):
            e_in = st(s, a=ex.a, hubble=ex.hubble, **arrays)
            for name in st.pingpong:
                arrays[name], arrays[f"{name}_next"] = \
                    arrays[f"{name}_next"], arrays[name]
                decomp.share_halos(arrays[name])
            ex.step(s, e_in["total"], e_in["pressure"], dt)
    if split:
        hc = torch.cat([arrays["hij_a"], arrays["hij_b"]])
        dhc = torch.cat([arrays["dhij_adt"], arrays["dhij_bdt"]])
    else:
        hc, dhc = arrays["hij"], arrays["dhijdt"]
    return (arrays["f"][cut].numpy(), arrays["dfdt"][cut].numpy(),
            hc[cut].numpy(), dhc[cut].numpy(),
            float(ex.a[0]), float(ex.adot[0]))


def check_gw_against_cpu(what, h, Stepper=ps.LowStorageRK54, split=False):
    f0, df0 = initial_data(GRID)
    h0, dh0 = initial_tensor_data(GRID)
    if Stepper is ps.LowStorageRK54:
        tableau = {}
    else:
        tableau = {"A": tuple(float(x) for x in Stepper._A),
                   "B": tuple(float(x) for x in Stepper._B)}
    fr, dfr, hr, dhr, ar, adr, energies = gw_reference(
        f0, df0, h0, dh0, DX, DT, STEPS, h, **tableau)
    fc, dfc, hc, dhc, ac, adc = cpu_gw_host_loop(
        f0, df0, h0, dh0, DX, DT, STEPS, h, Stepper=Stepper, split=split)
    assert len(energies) == Stepper.num_stages * STEPS + 1
    errs = {"f": np.abs(fc - fr).max(), "dfdt": np.abs(dfc - dfr).max(),
            "hij": np.abs(hc - hr).max(), "dhijdt": np.abs(dhc - dhr).max(),
            "a": abs(ac - ar) / abs(ar), "adot": abs(adc - adr) / abs(adr)}
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    tol = gw_tolerances()
    assert errs["f"] < 1e-14, errs
    assert errs["dfdt"] < 1e-14, errs
    assert errs["hij"] < tol["hij"], errs
    assert errs["dhijdt"] < tol["dhijdt"], errs
    assert errs["a"] < 1e-14, errs
    assert errs["adot"] < 1e-14, errs


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_gw_reference_matches_cpu_host_loop(h):
    check_gw_against_cpu(f"gw h={h}", h)


def test_gw_reference_matches_split_families():
    """Two three-component tensor families that are views of one parent
    (bench.py --gws-split), against the six-component reference."""
    check_gw_against_cpu("gw split h=2", 2, split=True)


@pytest.mark.parametrize("name", ["LowStorageRK3Williamson",
                                  "LowStorageRK3SSP", "LowStorageRK144"])
def test_gw_reference_matches_other_tableaus(name):
    """The tableaus the GPU matrix runs besides RK54, at its h = 2."""
    check_gw_against_cpu(f"gw {name} h=2", 2, Stepper=getattr(ps, name))


def test_gw_reference_leaves_scalars_alone():
    """The tensor sector does not back-react: gw_reference's scalar and
    Friedmann results are those of preheat_reference, bit for bit, with
    and without tensor data."""
    f0, df0 = initial_data(GRID)
    h0, dh0 = initial_tensor_data(GRID)
    fr, dfr, ar, adr, energies = preheat_reference(f0, df0, DX, DT, STEPS, 2)
    for tensor in ((h0, dh0), (None, None)):
        fg, dfg, hg, dhg, ag, adg, eg = gw_reference(
            f0, df0, *tensor, DX, DT, STEPS, 2)
        assert np.array_equal(fg, fr) and np.array_equal(dfg, dfr)
        assert (ag, adg) == (ar, adr)
        assert eg == energies
        assert (hg is None) == (tensor[0] is None)


def test_gw_reference_sensitivity():
    """What keeps the GPU matrix from being blind: every deliberately
    wrong variant of the reference moves at least one compared array by
    at least 1000 x the tolerance the GPU matrix holds that array to."""
    f0, df0 = initial_data(GRID)
    h0, dh0 = initial_tensor_data(GRID)
    tol = gw_tolerances()
    good = gw_reference(f0, df0, h0, dh0, DX, DT, STEPS, 2)
    for mutant in ("no_source", "swap_source", "grad_z_off", "no_friction",
                   "stale_k", "skip_site"):
        bad = gw_reference(f0, df0, h0, dh0, DX, DT, STEPS, 2,
                           _mutant=mutant)
        ratios = {"hij": np.abs(bad[2] - good[2]).max() / tol["hij"],
                  "dhijdt": np.abs(bad[3] - good[3]).max() / tol["dhijdt"]}
        print(f"{mutant}: " + ", ".join(
            f"{k} moved {v:.3g} x tol" for k, v in ratios.items()))
        # the scalars are compared too, and no mutant touches them
        assert np.array_equal(bad[0], good[0])
        assert max(ratios.values()) >= 1000, (mutant, ratios)


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

"""The fused register-ring kernels (backend/hip.py JitLapStage,
JitLapReduction) on float32 fields, with float64 reductions and a
float64 Friedmann ODE: every candidate tile, in-kernel periodic reads
on and off, every halo order and every region-split launch form, as
tests/test_stage_variants.py runs them in float64.

Yardstick: the float64 numpy integration of tests/preheat_reference.py
started from the same float32-rounded values, so that only the
arithmetic differs.  Tolerances (``TOL_FP32``): four times the deviation
of the float32 numpy emulation of tests/preheat_emulation_fp32.py from
that reference (f 6.2e-8, dfdt 4.9e-7, a 3.5e-11, adot 7.5e-9,
E 2.0e-8, P 2.4e-8 over h = 1..4); tests/test_stage_fp32_cpu.py pins
the emulation to a quarter of them.  The data is zero-mean (0.05
randn): one wrong neighbour in a single z-plane at the outermost,
smallest coefficient moves dfdt by 5.9e-6 (h=4), 3.6e-5 (h=3) and
3.6e-3 (h=1); one dropped site moves E by 1.6e-5.

The cancellation tests use data with the inflaton's 0.193 mean, where
a float32 Laplacian in the plain form ``c0*f0 + sum c_s (f+ + f-)``
fails by orders of magnitude (its inexact coefficients do not sum to
zero); their bounds are four times the difference-form emulation's
deviation.
"""

import functools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend.hip import JitLapReduction, JitLapStage
from pystella_amd.sectors import get_rho_and_p
from tests.preheat_emulation_fp32 import (
    TOL_FP32, deviations, zero_mean_data)
from tests.preheat_reference import (
    MPL, fd_reference, initial_data, potential, preheat_reference)
from tests.test_stage_variants import KNOBS, LAUNCH_FORMS

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

GRID = (72, 11, 80)
DX = (5 / 12, 5 / 11, 5 / 13)
DT = 1e-3
STEPS = 2

TILES = tuple(JitLapStage.TILE_CANDIDATES)


def _data(kind):
    if kind == "zero_mean":
        return zero_mean_data(GRID)
    f0, df0 = initial_data(GRID)
    return f0.astype(np.float32), df0.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(h, kind="zero_mean"):
    """One float64 numpy integration per halo order and data set,
    shared by every case."""
    f0, df0 = _data(kind)
    out = preheat_reference(f0, df0, DX, DT, STEPS, h)
    for arr in out[:2]:
        arr.setflags(write=False)
    return out


def _scalar(x):
    return float(np.asarray(x).reshape(-1)[0])


def _periodic_pad(u, h):
    return np.pad(u, ((0, 0),) + ((h, h),) * 3, mode="wrap")


def run_fp32(monkeypatch, h, tile, periodic, split=False, knobs=None,
             kind="zero_mean"):
    """Two device-resident RK54 steps on float32 arrays with the stage
    kernel forced to ``tile`` / ``periodic``; returns the deviations
    from the float64 reference (printed), and the loop."""
    from pystella_amd.fusion import (
        DeviceFriedmannLoop, FusedLaplacianReduction, StencilRKStepper)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PYSTELLA_TILE", ",".join(str(t) for t in tile))
    monkeypatch.setenv("PYSTELLA_PERIODIC", periodic)
    for name, value in (knobs or {}).items():
        monkeypatch.setenv(name, value)

    f0, df0 = _data(kind)
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    pad = tuple(n + 2 * h for n in GRID)
    cut = (slice(None),) + (slice(h, -h),) * 3
    f = torch.zeros((2,) + pad, dtype=torch.float32)
    dfdt = torch.zeros_like(f)
    f[cut] = torch.as_tensor(f0)
    dfdt[cut] = torch.as_tensor(df0)

    st = StencilRKStepper(ps.LowStorageRK54, [sector], derivs,
                          halo_shape=h, rank_shape=GRID, dt=DT,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=GRID, grid_size=gsize, store_lap=False)
    arrays = {"f": f.cuda(), "dfdt": dfdt.cuda()}
    arrays["f_next"] = torch.zeros_like(arrays["f"])

    # the seed energy: JitLapReduction, fixed (64,4,64) tile
    e0 = red(f=arrays["f"], dfdt=arrays["dfdt"], a=np.ones(1))
    assert isinstance(red._fused_kernel, JitLapReduction)
    assert red._fused_kernel.dtype == torch.float32
    energies = {0: (_scalar(e0["total"]), _scalar(e0["pressure"]))}

    ex = ps.Expansion(e0["total"], ps.LowStorageRK54, mpl=MPL)
    decomp.share_halos(arrays["f"])
    dl = DeviceFriedmannLoop(st, decomp, ex, gsize, DT, mpl=MPL)
    if split:
        nx, ny, nz = GRID

        def fake_regions(rank_shape, split_axes=None):
            interior = (h, nx - h, h, ny - h, h, nz - h)
            slabs = [
                (0, h, 0, ny, 0, nz),
                (nx - h, nx, 0, ny, 0, nz),
                (h, nx - h, 0, h, 0, nz),
                (h, nx - h, ny - h, ny, 0, nz),
                (h, nx - h, h, ny - h, 0, h),
                (h, nx - h, h, ny - h, nz - h, nz),
            ]
            return interior, slabs

        dl._regions = fake_regions

    for n in range(STEPS):
        dl.step(arrays)
        state = dl.read_state()
        energies[5 * n + 4] = (float(state["energy"]),
                               float(state["pressure"]))
        if n == 0:
            # the knobs took, and the kernels are the float32 ones
            want_per = (periodic == "1",) * 3
            for s in range(st.num_stages):
                for kern in st._stepper.steps[s]._hip_kernel:
                    assert isinstance(kern, JitLapStage)
                    assert kern.dtype == torch.float32
                    assert "using real = float;" in kern.source
                    assert tuple(kern.tile) == tuple(tile), \
                        (s, kern.tile, tile)
                    assert tuple(kern.periodic) == want_per, \
                        (s, kern.periodic, want_per)
    torch.cuda.synchronize()

    # float32 arrays on return, float64 state and sums
    for name in ("f", "f_next", "dfdt"):
        assert arrays[name].dtype == torch.float32, name
    tmps = st.tmp_arrays
    assert set(tmps) == {"f_tmp", "dfdt_tmp"}
    for name, t in tmps.items():
        assert t.dtype == torch.float32, name
    assert dl.state.dtype == torch.float64
    assert dl._sums.dtype == torch.float64

    fg = arrays["f"].cpu()[cut].numpy()
    dfg = arrays["dfdt"].cpu()[cut].numpy()
    assert np.isfinite(fg).all() and np.isfinite(dfg).all()
    dev = deviations(
        (fg, dfg, float(state["a"]), float(state["adot"]), energies),
        reference(h, kind), STEPS)
    print("    " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    return dev, dl


def run_and_check(monkeypatch, h, tile, periodic, **kwargs):
    dev, dl = run_fp32(monkeypatch, h, tile, periodic, **kwargs)
    for key, tol in TOL_FP32.items():
        assert dev[key] < tol, (key, dev[key], tol)
    return dl


def _tid(tile):
    return "x".join(str(t) for t in tile)


@requires_gpu
@pytest.mark.parametrize("periodic", ["0", "1"])
@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_fp32_stage_tile_matrix(tile, periodic, monkeypatch):
    """Every candidate tile x in-kernel periodic reads on/off, h=2."""
    run_and_check(monkeypatch, 2, tile, periodic)


@requires_gpu
@pytest.mark.parametrize("periodic", ["0", "1"])
@pytest.mark.parametrize("h", [1, 3, 4])
def test_fp32_stage_halo_orders(h, periodic, monkeypatch):
    """The other halo orders at the largest tile."""
    run_and_check(monkeypatch, h, TILES[0], periodic)


@requires_gpu
@pytest.mark.parametrize("form", list(LAUNCH_FORMS))
def test_fp32_stage_region_split_forms(form, monkeypatch):
    """Interior + six boundary slabs in each launch form, with filled
    halos really consumed (no in-kernel periodic reads)."""
    dl = run_and_check(monkeypatch, 2, TILES[1], "0", split=True,
                       knobs=LAUNCH_FORMS[form])
    interior, slabs = dl._boxes
    assert len(slabs) == 6
    assert len(dl._nblks) == (2 if form == "shell" else 7), dl._nblks


@requires_gpu
def test_fp32_mixed_dtypes_refused_before_launch(monkeypatch):
    """float32 f with float64 dfdt: TypeError from the seed reduction,
    the host-loop stage and the device loop, nothing launched."""
    from pystella_amd.backend import hip
    from pystella_amd.fusion import (
        DeviceFriedmannLoop, FusedLaplacianReduction, StencilRKStepper)
    h = 2
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    pad = tuple(n + 2 * h for n in GRID)
    st = StencilRKStepper(ps.LowStorageRK54, [sector], derivs,
                          halo_shape=h, rank_shape=GRID, dt=DT,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=GRID, grid_size=gsize, store_lap=False)
    arrays = {
        "f": torch.zeros((2,) + pad, dtype=torch.float32, device="cuda"),
        "dfdt": torch.zeros((2,) + pad, dtype=torch.float64,
                            device="cuda")}
    arrays["f_next"] = torch.zeros_like(arrays["f"])

    launched = []
    real_ext = hip.ext()

    class Spy:
        def __getattr__(self, name):
            if name == "jit_launch":
                launched.append(name)
            return getattr(real_ext, name)

    monkeypatch.setattr(hip, "ext", lambda: Spy())
    with pytest.raises(TypeError, match="dfdt"):
        red(f=arrays["f"], dfdt=arrays["dfdt"], a=np.ones(1))
    with pytest.raises(TypeError, match="dfdt"):
        st(0, a=np.ones(1), hubble=np.zeros(1), **arrays)
    ex = ps.Expansion(1.0, ps.LowStorageRK54, mpl=MPL)
    dl = DeviceFriedmannLoop(st, decomp, ex, gsize, DT, mpl=MPL)
    with pytest.raises(TypeError, match="dfdt"):
        dl.step(arrays)
    assert not launched

    # a float32 kernel handed a float64 array names the argument
    arrays["dfdt"] = arrays["dfdt"].float()
    kerns = st._stepper.steps[0].ring_kernels(GRID, torch.float32)
    env = dict(arrays, dt=DT, rk_a0=0.0, a=1.0, hubble=0.0,
               f_tmp=torch.zeros((2,) + GRID, device="cuda"),
               dfdt_tmp=torch.zeros((2,) + GRID, dtype=torch.float64,
                                    device="cuda"))
    with pytest.raises(TypeError, match="argument dfdt_tmp has dtype "
                       "torch.float64"):
        kerns[0](env)
    assert not launched


# -- cancellation safety --------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("h", [2, 4])
def test_fp32_stored_laplacian_cancels_the_mean(h):
    """float32(0.193 + 1e-6 randn): the Laplacian's whole signal is
    2e-4.  Max abs error against the float64-accumulated stencil of
    the same float32 input <= 1.5e-10 (four times the difference form's
    3.9e-11 / 4.2e-11 in the emulation; the plain form gives 2e-6)."""
    from pystella_amd.fusion import FusedLaplacianReduction
    rng = np.random.default_rng(1)
    u = (0.193 + 1e-6 * rng.standard_normal((2,) + GRID)).astype(
        np.float32)
    upad = _periodic_pad(u, h)
    want = fd_reference(upad, h, DX)[0]
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=GRID, grid_size=gsize, store_lap=True)
    f = torch.as_tensor(upad).cuda()
    dfdt = torch.zeros_like(f)
    lap = torch.full((2,) + GRID, float("nan"), dtype=torch.float32,
                     device="cuda")
    red(f=f, dfdt=dfdt, lap_f=lap, a=np.ones(1))
    assert red._fused_kernel.dtype == torch.float32
    got = lap.cpu().numpy()
    assert got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"    h={h}: max|lap| {np.abs(want).max():.3e}  "
          f"max abs err {err:.3e}")
    assert err <= 1.5e-10, err


@requires_gpu
@pytest.mark.parametrize("h", [2, 4])
def test_fp32_full_loop_cancels_the_mean(h, monkeypatch):
    """Two RK54 steps from initial_data (0.193 mean, 1e-3 fluctuations)
    rounded to float32: E and P within 1.2e-8, adot within 5e-9, a
    within 5e-12 (four times the difference-form emulation's 2.8e-9,
    2.6e-9, 1.1e-9, 1.1e-12; the plain form gives 9e-7 in E)."""
    dev, _ = run_fp32(monkeypatch, h, TILES[0], "1", kind="preheating")
    assert dev["E"] <= 1.2e-8 and dev["P"] <= 1.2e-8, dev
    assert dev["adot"] <= 5e-9, dev
    assert dev["a"] <= 5e-12, dev


# -- the six-component tensor family with inline gradients ---------------

def _gw_run(dtype, device, nsteps=2):
    """(arrays, a) after ``nsteps`` RK54 steps of scalar + h_ij sectors
    on (16,16,16): the torch host loop on the CPU, the device-resident
    loop on the GPU."""
    from pystella_amd.fusion import (
        DeviceFriedmannLoop, FusedLaplacianReduction, StencilRKStepper)
    grid = (16, 16, 16)
    h = 2
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=grid)
    dx = (0.3, 0.3, 0.3)
    dt = 0.005
    gsize = float(np.prod(grid))
    sector = ps.ScalarSector(2, potential=lambda f: f[0]**2 / 2)
    tensor = ps.TensorPerturbationSector([sector])
    derivs = ps.FiniteDifferencer(decomp, h, dx, rank_shape=grid)
    pad = tuple(n + 2 * h for n in grid)
    rng = np.random.default_rng(51)

    def rand(n, mean, amp):
        x = (mean + amp * rng.standard_normal((n,) + pad)).astype(
            np.float32)
        return torch.as_tensor(x).to(dtype).to(device)

    arrays = {"f": rand(2, 0.2, 0.01), "dfdt": rand(2, 0.0, 0.01),
              "hij": rand(6, 0.0, 0.05), "dhijdt": rand(6, 0.0, 0.05)}
    arrays["f_next"] = torch.zeros_like(arrays["f"])
    arrays["hij_next"] = torch.zeros_like(arrays["hij"])
    st = StencilRKStepper(ps.LowStorageRK54, [sector, tensor], derivs,
                          halo_shape=h, rank_shape=grid, dt=dt,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p, inline_grad=True)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=grid, grid_size=gsize, store_lap=False)
    for name in st.pingpong:
        decomp.share_halos(arrays[name])
    e0 = red(f=arrays["f"], dfdt=arrays["dfdt"], a=np.ones(1))
    ex = ps.Expansion(e0["total"], ps.LowStorageRK54)
    if device == "cuda":
        dl = DeviceFriedmannLoop(st, decomp, ex, gsize, dt)
        for _ in range(nsteps):
            dl.step(arrays)
        a = float(dl.read_state()["a"])
        kerns = [k for s in range(st.num_stages)
                 for k in st._stepper.steps[s]._hip_kernel]
        assert {k.nf for k in kerns} == {2, 6}
        assert all(k.dtype == dtype for k in kerns)
    else:
        for _ in range(nsteps):
            for s in range(st.num_stages):
                e_in = st(s, a=ex.a, hubble=ex.hubble, **arrays)
                for name in st.pingpong:
                    arrays[name], arrays[f"{name}_next"] = \
                        arrays[f"{name}_next"], arrays[name]
                    decomp.share_halos(arrays[name])
                ex.step(s, e_in["total"], e_in["pressure"], dt)
        a = float(ex.a[0])
    cut = (slice(None),) + (slice(h, -h),) * 3
    out = {k: arrays[k].cpu()[cut].double().numpy()
           for k in ("f", "dfdt", "hij", "dhijdt")}
    for k in ("f", "dfdt", "hij", "dhijdt"):
        assert arrays[k].dtype == dtype, k
    return out, a


@requires_gpu
def test_fp32_gw_family(monkeypatch):
    """nf = 6 h_ij family with inline gradients in float32 against the
    torch-CPU host path in float64.  Tolerance, per array: four times
    the deviation of that same CPU path run in float32 (same rounded
    initial values) from its float64 run."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    ref, a_ref = _gw_run(torch.float64, "cpu")
    cpu32, a_cpu32 = _gw_run(torch.float32, "cpu")
    gpu32, a_gpu32 = _gw_run(torch.float32, "cuda")
    torch.cuda.synchronize()
    for k in ("f", "dfdt", "hij", "dhijdt"):
        tol = 4 * np.abs(cpu32[k] - ref[k]).max()
        err = np.abs(gpu32[k] - ref[k]).max()
        print(f"    {k}: cpu32 dev {tol / 4:.3e}  tol {tol:.3e}  "
              f"gpu32 err {err:.3e}  max|x| {np.abs(ref[k]).max():.3e}")
        assert np.isfinite(gpu32[k]).all()
        assert tol > 0 and err <= tol, (k, err, tol)
    tol_a = 4 * abs(a_cpu32 - a_ref) / a_ref
    err_a = abs(a_gpu32 - a_ref) / a_ref
    print(f"    a: cpu32 dev {tol_a / 4:.3e}  gpu32 err {err_a:.3e}")
    assert err_a <= max(tol_a, 4 * 2.0 ** -53), (err_a, tol_a)

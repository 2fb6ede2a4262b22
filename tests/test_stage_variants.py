"""The fused register-ring RK stage kernel (backend/hip.py JitLapStage)
at every candidate tile, with and without in-kernel periodic reads, at
every halo order and in every region-split launch form — each compared
with the independent numpy integration of tests/preheat_reference.py
(pinned against the CPU host loop by tests/test_preheat_reference.py).

The grid (72, 11, 80) gives every candidate tile at least two z-blocks
with a 16-lane last block, several x-chunks with a short last chunk
(except (32,2,8), where 72 divides exactly) and, for every tile but
(64,4,32), a short last y-tile, so the periodic wrap crosses chunk and
block seams.  Two full RK54 steps are run: the elided last-stage
k-stores are observable only through the next step's stage 0.

Tolerances are those tests/test_crosscheck.py holds the same
comparison to.  One dropped or double-counted site moves E by ~1.6e-5
relative; one wrong stencil neighbour moves dfdt by ~1e-7.
"""

import functools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend.hip import JitLapStage
from pystella_amd.sectors import get_rho_and_p
from tests.preheat_reference import (
    MPL, gw_reference, initial_data, potential, preheat_reference)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

GRID = (72, 11, 80)
DX = (5 / 12, 5 / 11, 5 / 13)
DT = 1e-3
STEPS = 2

TILES = tuple(JitLapStage.TILE_CANDIDATES)
KNOBS = ("PYSTELLA_TILE", "PYSTELLA_PERIODIC", "PYSTELLA_SHELL",
         "PYSTELLA_SLAB_TILES", "PYSTELLA_SLAB_STREAMS",
         "PYSTELLA_NO_OVERLAP", "PYSTELLA_WRAP_OVERLAP",
         "PYSTELLA_SECTIONS", "PYSTELLA_KEEP_LASTK")


def tableau(stepper):
    """The ``(A, B)`` arguments of the reference for the framework's
    ``stepper`` class: RK54 keeps the reference's own literal table."""
    if stepper == "LowStorageRK54":
        return {}
    cls = getattr(ps, stepper)
    return {"A": tuple(float(x) for x in cls._A),
            "B": tuple(float(x) for x in cls._B)}


@functools.lru_cache(maxsize=None)
def reference(h, stepper="LowStorageRK54"):
    """One numpy integration per halo order (and tableau), shared by
    every case."""
    f0, df0 = initial_data(GRID)
    if stepper == "LowStorageRK54":
        out = preheat_reference(f0, df0, DX, DT, STEPS, h)
    else:
        fr, dfr, _, _, ar, adr, energies = gw_reference(
            f0, df0, None, None, DX, DT, STEPS, h, **tableau(stepper))
        out = fr, dfr, ar, adr, energies
    for arr in out[:2]:
        arr.setflags(write=False)
    return out


def _scalar(x):
    return float(np.asarray(x).reshape(-1)[0])


def _check_energy(what, E, P, Er, Pr):
    eE = abs(E - Er) / abs(Er)
    eP = abs(P - Pr) / max(abs(Pr), abs(Er))
    print(f"    {what}: E rel {eE:.3e}  P rel {eP:.3e}")
    assert eE < 1e-10, (what, E, Er)
    assert eP < 1e-10, (what, P, Pr)


def run_and_check(monkeypatch, h, tile, periodic, split=False, knobs=None,
                  stepper="LowStorageRK54"):
    """Two device-resident steps of the 2N-storage ``stepper`` with the
    stage kernel forced to ``tile`` / ``periodic``; every compared
    quantity is printed, then asserted against the numpy reference."""
    from pystella_amd.fusion import (
        DeviceFriedmannLoop, FusedLaplacianReduction, StencilRKStepper)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PYSTELLA_TILE", ",".join(str(t) for t in tile))
    monkeypatch.setenv("PYSTELLA_PERIODIC", periodic)
    for name, value in (knobs or {}).items():
        monkeypatch.setenv(name, value)

    Stepper = getattr(ps, stepper)
    ns = Stepper.num_stages
    fr, dfr, ar, adr, energies = reference(h, stepper)
    f0, df0 = initial_data(GRID)
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    pad = tuple(n + 2 * h for n in GRID)
    cut = (slice(None),) + (slice(h, -h),) * 3
    f = torch.zeros((2,) + pad, dtype=torch.float64)
    dfdt = torch.zeros_like(f)
    f[cut] = torch.as_tensor(f0)
    dfdt[cut] = torch.as_tensor(df0)

    st = StencilRKStepper(Stepper, [sector], derivs,
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
    _check_energy("seed reduction", _scalar(e0["total"]),
                  _scalar(e0["pressure"]), *energies[0])

    ex = ps.Expansion(e0["total"], Stepper, mpl=MPL)
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

    states = []
    for n in range(STEPS):
        dl.step(arrays)
        states.append(dl.read_state())
        if n == 0:
            # the knobs took: a silently ignored one would turn the
            # matrix into copies of one case
            want_per = (periodic == "1",) * 3
            for s in range(st.num_stages):
                for kern in st._stepper.steps[s]._hip_kernel:
                    assert isinstance(kern, JitLapStage)
                    assert tuple(kern.tile) == tuple(tile), \
                        (s, kern.tile, tile)
                    assert tuple(kern.periodic) == want_per, \
                        (s, kern.periodic, want_per)
    torch.cuda.synchronize()

    # per-step (E, P): the pair fed to the last stage's Friedmann update
    for n, state in enumerate(states):
        _check_energy(f"step {n} last stage", float(state["energy"]),
                      float(state["pressure"]),
                      *energies[ns * n + ns - 1])

    fg = arrays["f"].cpu()[cut].numpy()
    dfg = arrays["dfdt"].cpu()[cut].numpy()
    a, adot = float(states[-1]["a"]), float(states[-1]["adot"])
    ef = np.abs(fg - fr).max()
    edf = np.abs(dfg - dfr).max()
    ea = abs(a - ar) / abs(ar)
    ead = abs(adot - adr) / abs(adr)
    print(f"    final: f abs {ef:.3e}  dfdt abs {edf:.3e}  "
          f"a rel {ea:.3e}  adot rel {ead:.3e}")
    assert np.isfinite(fg).all() and np.isfinite(dfg).all()
    assert ef < 1e-12, ef
    assert edf < 1e-10, edf
    assert ea < 1e-13, (a, ar)
    assert ead < 1e-12, (adot, adr)
    return dl


def _tid(tile):
    return "x".join(str(t) for t in tile)


@requires_gpu
@pytest.mark.parametrize("periodic", ["0", "1"])
@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_stage_tile_matrix(tile, periodic, monkeypatch):
    """Every candidate tile x in-kernel periodic reads on/off, h=2."""
    run_and_check(monkeypatch, 2, tile, periodic)


@requires_gpu
@pytest.mark.parametrize("periodic", ["0", "1"])
@pytest.mark.parametrize("tile", (TILES[0], TILES[-1]), ids=_tid)
@pytest.mark.parametrize("h", [1, 3, 4])
def test_stage_halo_orders(h, tile, periodic, monkeypatch):
    """The other halo orders at the largest and the smallest tile."""
    run_and_check(monkeypatch, h, tile, periodic)


LAUNCH_FORMS = {
    "shell": {},
    "slabs": {"PYSTELLA_SHELL": "0"},
}


@requires_gpu
@pytest.mark.parametrize("form", list(LAUNCH_FORMS))
@pytest.mark.parametrize("tile", (TILES[0], TILES[-1]), ids=_tid)
def test_stage_region_split_forms(tile, form, monkeypatch):
    """Interior + six boundary slabs (the geometry of a rank of a
    (2,2,2) decomposition) in each launch form, with filled halos
    really consumed (no in-kernel periodic reads)."""
    dl = run_and_check(monkeypatch, 2, tile, "0", split=True,
                       knobs=LAUNCH_FORMS[form])
    interior, slabs = dl._boxes
    assert len(slabs) == 6
    # the split really happened: one launch group per region
    assert len(dl._nblks) == (2 if form == "shell" else 7), dl._nblks


@requires_gpu
@pytest.mark.parametrize("periodic", ["0", "1"])
def test_stage_rk144(periodic, monkeypatch):
    """A fourteen-stage 2N tableau through the stage kernels and the
    device loop at the smallest tile: the last-stage k-store elision
    keys on ``num_stages`` and ``_A[0] == 0``, not on RK54."""
    run_and_check(monkeypatch, 2, TILES[-1], periodic,
                  stepper="LowStorageRK144")

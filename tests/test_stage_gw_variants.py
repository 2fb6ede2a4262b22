"""The fused register-ring RK stage kernels (backend/hip.py JitLapStage)
in their gravitational-wave forms — the two-scalar family next to a
six-component ``h_ij`` family, or next to two three-component families
that are views of one parent — at every candidate tile, halo order,
launch form and 2N-storage tableau, each compared with
``gw_reference`` of tests/preheat_reference.py: a plain-numpy
integration that shares no code with the framework (no symbolic
equations, no ``TensorPerturbationSector``, no ``tensor_index``, no
``centered_diff``, no tableau plumbing).
tests/test_preheat_reference.py pins that reference against the CPU
host loop and shows that it is sensitive: a dropped or swapped source
component, a gradient read one site off, a dropped friction term, a
stale k and a single skipped site each move ``hij`` or ``dhijdt`` by
more than 1000 x the tolerances used here.

Grid, spacings, time step and the partial-tile reasoning are those of
tests/test_stage_variants.py.  The ``*_next`` buffers start as NaN over
the whole padded array: the stage kernels must write every interior
site and every halo must be wrapped before it is read (the ``h_ij``
kernel's inlined gradients read ``f`` halos through the generic
codegen), so a surviving NaN is a dropped site or an unfilled halo.
The k arrays stay as the stepper allocates them (zeros): 0 x NaN would
poison stage 0.

Tolerances.  ``f``, ``dfdt``, ``a``, ``adot`` and the per-step (E, P)
are held to exactly what tests/test_stage_variants.py holds them to;
the tensor sector does not back-react, so the scalar reference values
are those of ``preheat_reference`` bit for bit (asserted).  ``hij`` and
``dhijdt`` get the relative allowance that file gives ``f``
(1e-12 / max|f| ~ 5e-12) and ``dfdt`` (1e-10 / max|dfdt| ~ 7e-10),
scaled to the reference arrays' magnitudes (max|hij| ~ 4.7e-3,
max|dhijdt| ~ 5e-3): 2.5e-14 and 3.5e-12 absolute.  The CPU host loop
agrees with the reference to 9e-19 and 8e-18; the smallest mutant
effect is 6.7e-9 in ``hij`` (stale k) and 1.2e-8 in ``dhijdt``.

Measured on an MI355X (maxima over the cases of each test; every case
gave ``f`` <= 5.6e-17, ``dfdt`` <= 8.4e-17, ``a`` 0 and ``adot``
<= 6.5e-16 relative — the figures of the CPU host loop):

    test                              hij abs    dhijdt abs
    test_gw_tile_matrix               4.3e-19    1.3e-18
    test_gw_halo_orders       h=1     4.3e-19    8.7e-19
                              h=3     4.3e-19    1.3e-18
                              h=4     4.3e-19    1.7e-18
    test_gw_region_split_forms        4.3e-19    1.3e-18
    test_gw_periodic_request_...      4.3e-19    1.3e-18
    test_gw_split_families            4.3e-19    1.3e-18
    test_gw_split_families_keep_lastk 4.3e-19    1.3e-18
    test_gw_tableaus                  4.3e-19    8.7e-19
    test_gw_host_launched             4.3e-19    1.3e-18

so the tolerances stand four orders above the kernels' deviation and
more than five below the smallest mutant effect.  A case costs 1.0 to
2.5 s (ten hiprtc compiles for RK54) next to 0.65 to 0.85 s for its
two-scalar counterpart, so every sub-matrix stays on RK54.
"""

import functools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend.hip import JitLapStage
from pystella_amd.sectors import get_rho_and_p
from pystella_amd.step import _field_of
from tests.preheat_reference import (
    MPL, gw_reference, initial_data, initial_tensor_data, potential)
from tests.test_stage_variants import (
    DT, DX, GRID, KNOBS, LAUNCH_FORMS, STEPS, TILES, _check_energy, _scalar,
    _tid, reference, tableau)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

TOL_HIJ = 2.5e-14
TOL_DHIJDT = 3.5e-12

# the tableau of the halo-order, launch-form, split-family and
# host-launched sub-matrices (the tile matrix is always RK54)
SUB_STEPPER = "LowStorageRK54"


@functools.lru_cache(maxsize=None)
def gw_ref(h, stepper="LowStorageRK54"):
    """One numpy integration per (halo order, tableau), shared by every
    case and read-only."""
    f0, df0 = initial_data(GRID)
    h0, dh0 = initial_tensor_data(GRID)
    out = gw_reference(f0, df0, h0, dh0, DX, DT, STEPS, h,
                       **tableau(stepper))
    for arr in out[:4]:
        arr.setflags(write=False)
    # no back-reaction: the scalar and Friedmann values are those the
    # scalar matrix compares with
    fr, dfr, ar, adr, energies = reference(h, stepper)
    assert np.array_equal(out[0], fr) and np.array_equal(out[1], dfr)
    assert (out[4], out[5]) == (ar, adr) and out[6] == energies
    return out


def _k_stores(fam):
    """Names of the k arrays the ring family's statements store to."""
    names = {_field_of(key)[0].name for key in fam.rk}
    return {n for n in names if n.endswith("_tmp")}


def run_gw(monkeypatch, h, tile, stepper="LowStorageRK54", families="six",
           form="device", regions=False, periodic=None, knobs=None):
    """Two steps of scalars + tensor perturbations on the GPU with the
    stage kernels forced to ``tile``, every compared deviation printed
    and then asserted against the numpy reference.

    ``families``: ``"six"`` (one six-component family) or ``"split"``
    (two three-component families, views of one parent).  ``form``:
    ``"device"`` (DeviceFriedmannLoop.step) or ``"host"``
    (StencilRKStepper.__call__ per stage, scalars by value, no state
    buffer, Expansion.step on the host).  ``regions``: the interior +
    six boundary slabs of a rank of a (2,2,2) decomposition.
    Returns ``(stepper, device loop or None)``."""
    from pystella_amd.fusion import (
        DeviceFriedmannLoop, FusedLaplacianReduction, StencilRKStepper)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PYSTELLA_TILE", ",".join(str(t) for t in tile))
    if periodic is not None:
        monkeypatch.setenv("PYSTELLA_PERIODIC", periodic)
    for name, value in (knobs or {}).items():
        monkeypatch.setenv(name, value)

    Stepper = getattr(ps, stepper)
    ns = Stepper.num_stages
    fr, dfr, hr, dhr, ar, adr, energies = gw_ref(h, stepper)
    f0, df0 = initial_data(GRID)
    h0, dh0 = initial_tensor_data(GRID)
    gsize = float(np.prod(GRID))
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    sector = ps.ScalarSector(2, potential=potential)
    if families == "split":
        tensors = [
            ps.TensorPerturbationSector(
                [sector], components=(0, 1, 2), name="hij_a"),
            ps.TensorPerturbationSector(
                [sector], components=(3, 4, 5), name="hij_b")]
        want_nf = {2, 3}
    else:
        tensors = [ps.TensorPerturbationSector([sector])]
        want_nf = {2, 6}
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    pad = tuple(n + 2 * h for n in GRID)
    cut = (slice(None),) + (slice(h, -h),) * 3

    def padded(x):
        out = torch.zeros(x.shape[:1] + pad, dtype=torch.float64)
        out[cut] = torch.as_tensor(x)
        return out.cuda()

    f, dfdt, hij, dhijdt = (padded(x) for x in (f0, df0, h0, dh0))
    # poisoned targets: every interior site must be written, every halo
    # wrapped before it is read
    f_next = torch.full_like(f, float("nan"))
    hij_next = torch.full_like(hij, float("nan"))
    arrays = {"f": f, "dfdt": dfdt, "f_next": f_next}
    if families == "split":
        # views of one parent, as bench.py --gws-split builds them
        arrays.update({
            "hij_a": hij[0:3], "hij_b": hij[3:6],
            "hij_a_next": hij_next[0:3], "hij_b_next": hij_next[3:6],
            "dhij_adt": dhijdt[0:3], "dhij_bdt": dhijdt[3:6]})
    else:
        arrays.update({"hij": hij, "hij_next": hij_next, "dhijdt": dhijdt})

    st = StencilRKStepper(Stepper, [sector] + tensors, derivs,
                          halo_shape=h, rank_shape=GRID, dt=DT,
                          reducers=sector, grid_size=gsize,
                          callback=get_rho_and_p, inline_grad=True)
    red = FusedLaplacianReduction(
        decomp, sector, derivs, halo_shape=h, callback=get_rho_and_p,
        rank_shape=GRID, grid_size=gsize, store_lap=False)
    e0 = red(f=arrays["f"], dfdt=arrays["dfdt"], a=np.ones(1))
    _check_energy("seed reduction", _scalar(e0["total"]),
                  _scalar(e0["pressure"]), *energies[0])
    ex = ps.Expansion(e0["total"], Stepper, mpl=MPL)
    for name in st.pingpong:
        decomp.share_halos(arrays[name])

    def check_kernels():
        # the knobs took: a silently ignored one would turn the matrix
        # into copies of one case.  In-kernel periodic reads stay off
        # whatever was asked: the inlined gradients need filled halos.
        for s in range(ns):
            smap = st._stepper.steps[s]
            assert smap.needs_filled_halos
            assert {k.nf for k in smap._hip_kernel} == want_nf
            assert len(smap._hip_kernel) == len(tensors) + 1
            for kern in smap._hip_kernel:
                assert isinstance(kern, JitLapStage)
                assert tuple(kern.tile) == tuple(tile), (s, kern.tile)
                assert tuple(kern.periodic) == (False, False, False), \
                    (s, kern.periodic)

    dl = None
    if form == "device":
        dl = DeviceFriedmannLoop(st, decomp, ex, gsize, DT, mpl=MPL)
        if regions:
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
                check_kernels()
        torch.cuda.synchronize()
        # per-step (E, P): the pair fed to the last stage's Friedmann
        # update
        for n, state in enumerate(states):
            _check_energy(f"step {n} last stage", float(state["energy"]),
                          float(state["pressure"]),
                          *energies[ns * n + ns - 1])
        a, adot = float(states[-1]["a"]), float(states[-1]["adot"])
    else:
        assert not regions
        stage_energies = []
        for n in range(STEPS):
            for s in range(ns):
                e_in = st(s, a=ex.a, hubble=ex.hubble, **arrays)
                for name in st.pingpong:
                    arrays[name], arrays[f"{name}_next"] = \
                        arrays[f"{name}_next"], arrays[name]
                    decomp.share_halos(arrays[name])
                ex.step(s, e_in["total"], e_in["pressure"], DT)
                stage_energies.append((_scalar(e_in["total"]),
                                       _scalar(e_in["pressure"])))
            if n == 0:
                check_kernels()
        torch.cuda.synchronize()
        for n in range(STEPS):
            _check_energy(f"step {n} last stage",
                          *stage_energies[ns * n + ns - 1],
                          *energies[ns * n + ns - 1])
        a, adot = float(ex.a[0]), float(ex.adot[0])

    if families == "split":
        hg = torch.cat([arrays["hij_a"], arrays["hij_b"]])
        dhg = torch.cat([arrays["dhij_adt"], arrays["dhij_bdt"]])
    else:
        hg, dhg = arrays["hij"], arrays["dhijdt"]
    fg = arrays["f"].cpu()[cut].numpy()
    dfg = arrays["dfdt"].cpu()[cut].numpy()
    hg = hg.cpu()[cut].numpy()
    dhg = dhg.cpu()[cut].numpy()
    ef = np.abs(fg - fr).max()
    edf = np.abs(dfg - dfr).max()
    eh = np.abs(hg - hr).max()
    edh = np.abs(dhg - dhr).max()
    ea = abs(a - ar) / abs(ar)
    ead = abs(adot - adr) / abs(adr)
    print(f"    final: f abs {ef:.3e}  dfdt abs {edf:.3e}  "
          f"hij abs {eh:.3e}  dhijdt abs {edh:.3e}  "
          f"a rel {ea:.3e}  adot rel {ead:.3e}")
    for name, arr in (("f", fg), ("dfdt", dfg), ("hij", hg),
                      ("dhijdt", dhg)):
        assert np.isfinite(arr).all(), \
            (name, int((~np.isfinite(arr)).sum()))
    assert ef < 1e-12, ef
    assert edf < 1e-10, edf
    assert eh < TOL_HIJ, eh
    assert edh < TOL_DHIJDT, edh
    assert ea < 1e-13, (a, ar)
    assert ead < 1e-12, (adot, adr)
    return st, dl


@requires_gpu
@pytest.mark.parametrize("tile", TILES, ids=_tid)
def test_gw_tile_matrix(tile, monkeypatch):
    """Every candidate tile, h=2, RK54, six-component family."""
    run_gw(monkeypatch, 2, tile)


@requires_gpu
@pytest.mark.parametrize("tile", (TILES[0], TILES[-1]), ids=_tid)
@pytest.mark.parametrize("h", [1, 3, 4])
def test_gw_halo_orders(h, tile, monkeypatch):
    """The other halo orders at the largest and the smallest tile."""
    run_gw(monkeypatch, h, tile, stepper=SUB_STEPPER)


@requires_gpu
@pytest.mark.parametrize("form", list(LAUNCH_FORMS))
@pytest.mark.parametrize("tile", (TILES[0], TILES[-1]), ids=_tid)
def test_gw_region_split_forms(tile, form, monkeypatch):
    """Interior + six boundary slabs in each launch form: the ``h_ij``
    kernel's inlined gradients consume ``f`` halos that arrive between
    the interior and the boundary launches."""
    _, dl = run_gw(monkeypatch, 2, tile, stepper=SUB_STEPPER, regions=True,
                   knobs=LAUNCH_FORMS[form])
    interior, slabs = dl._boxes
    assert len(slabs) == 6
    # the split really happened: one launch group per region
    assert len(dl._nblks) == (2 if form == "shell" else 7), dl._nblks


@requires_gpu
def test_gw_periodic_request_is_refused(monkeypatch):
    """PYSTELLA_PERIODIC=1 with the tensor sector: the kernels must
    keep reading filled halos (run_gw asserts ``needs_filled_halos``
    and ``periodic == (False,)*3``) and the halos must still be
    wrapped; with in-kernel periodic reads the inlined gradients would
    read unwrapped (here: NaN) halos."""
    run_gw(monkeypatch, 2, TILES[1], periodic="1")


@requires_gpu
@pytest.mark.parametrize("tile", (TILES[0], TILES[-1]), ids=_tid)
def test_gw_split_families(tile, monkeypatch):
    """Two three-component families that are views of one parent
    (bench.py --gws-split): for these the last stage's k stores are
    elided, which only the second step's stage 0 can notice."""
    st, _ = run_gw(monkeypatch, 2, tile, stepper=SUB_STEPPER,
                   families="split")
    for fam in st._stepper.steps[-1].ring:
        assert fam.nf in (2, 3)
        assert not _k_stores(fam), (fam.f_name, _k_stores(fam))
    # ... and only the last stage's
    for smap in st._stepper.steps[:-1]:
        for fam in smap.ring:
            assert len(_k_stores(fam)) == 2, (fam.f_name, _k_stores(fam))


@requires_gpu
def test_gw_split_families_keep_lastk(monkeypatch):
    """The same with PYSTELLA_KEEP_LASTK=1: every stage stores k."""
    st, _ = run_gw(monkeypatch, 2, TILES[-1], stepper=SUB_STEPPER,
                   families="split", knobs={"PYSTELLA_KEEP_LASTK": "1"})
    for smap in st._stepper.steps:
        for fam in smap.ring:
            assert len(_k_stores(fam)) == 2, (fam.f_name, _k_stores(fam))


@requires_gpu
@pytest.mark.parametrize("stepper", ["LowStorageRK3Williamson",
                                     "LowStorageRK3SSP"])
def test_gw_tableaus(stepper, monkeypatch):
    """Other 2N-storage tableaus through the stage kernels, the device
    loop and the device Friedmann update, at the smallest tile; the
    Expansion and the reference use the same tableau."""
    run_gw(monkeypatch, 2, TILES[-1], stepper=stepper)


@requires_gpu
@pytest.mark.parametrize("tile", (TILES[0], TILES[-1]), ids=_tid)
def test_gw_host_launched(tile, monkeypatch):
    """StencilRKStepper.__call__ per stage: scalars by value, no state
    buffer, full-grid launches, Expansion.step on the host."""
    run_gw(monkeypatch, 2, tile, stepper=SUB_STEPPER, form="host")

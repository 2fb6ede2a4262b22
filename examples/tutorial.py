"""Executable walkthrough of the pystella_amd API (the runnable form
of docs/TUTORIAL.md; analogue of the reference's
examples/codegen-tutorial.ipynb).  Runs in a few seconds on CPU and
identically on an MI355X (--device cuda); every section prints what it
computed.  Covered: symbolic fields → elementwise/stencil kernels →
decomposition → time stepping → Fourier stack → multigrid → the fused
hot loop → HDF5 output/checkpointing.
"""

import argparse

import numpy as np
import torch

import pystella_amd as ps
from pystella_amd.field import DynamicField, Field, diff, shift_fields
from pystella_amd.sectors import get_rho_and_p


def main(args=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--n", type=int, default=16)
    p = ap.parse_args(args)
    device = torch.device(p.device)
    n, h = p.n, 2
    grid = (n, n, n)
    pad = tuple(m + 2 * h for m in grid)
    L = 5.0
    dx = (L / n,) * 3
    dk = (2 * np.pi / L,) * 3
    dt = 0.1 * min(dx)

    # -- 1. fields and expressions -------------------------------------
    f = DynamicField("f", offset="h", shape=(2,))
    H = Field("hubble", indices=[])
    V = f[0] ** 2 / 2 + f[0] ** 2 * f[1] ** 2 / 4
    dV0 = diff(V, f[0])
    eom = f.lap[0] - 2 * H * f.dot[0] - dV0
    print("1. symbolic EOM built:", type(eom).__name__)

    # -- 2. elementwise map + stencil ----------------------------------
    g = Field("g", offset=0)
    rho_map = ps.ElementWiseMap({g: f.dot[0] ** 2 / 2 + V},
                                halo_shape=h, rank_shape=grid)
    torch.manual_seed(0)
    f_arr = torch.rand((2,) + pad, dtype=torch.float64, device=device)
    dfdt_arr = torch.rand((2,) + pad, dtype=torch.float64,
                          device=device)
    g_arr = torch.zeros(grid, dtype=torch.float64, device=device)
    rho_map(f=f_arr, dfdt=dfdt_arr, g=g_arr, hubble=0.1)
    print("2. elementwise map:", float(g_arr.mean()))

    s_in = Field("sin_f", offset="h")
    s_out = Field("sout", offset=0)
    st = ps.Stencil({s_out: (shift_fields(s_in, (1, 0, 0))
                             + shift_fields(s_in, (-1, 0, 0))
                             + shift_fields(s_in, (0, 1, 0))
                             + shift_fields(s_in, (0, -1, 0))) / 4},
                    halo_shape=h, rank_shape=grid)
    sarr = torch.rand(pad, dtype=torch.float64, device=device)
    sout = torch.zeros(grid, dtype=torch.float64, device=device)
    st(sin_f=sarr, sout=sout)
    print("2b. stencil avg:", float(sout.mean()))

    # -- 3. decomposition ----------------------------------------------
    ps.init_distributed()
    decomp = ps.DomainDecomposition((1, 1, 1), h, grid_shape=grid)
    decomp.share_halos(f_arr)
    total = decomp.allreduce(float(f_arr[:, h:-h, h:-h, h:-h].sum()))
    print("3. halos shared; allreduced sum:", round(total, 3))

    # -- 4. reference-structure time stepping --------------------------
    sector = ps.ScalarSector(2, potential=lambda ff: (
        ff[0] ** 2 / 2 + ff[0] ** 2 * ff[1] ** 2 / 4))
    stepper = ps.LowStorageRK54([sector], dt=dt, halo_shape=h,
                                rank_shape=grid)
    derivs = ps.FiniteDifferencer(decomp, h, dx, rank_shape=grid)
    red = ps.Reduction(decomp, sector, halo_shape=h,
                       callback=get_rho_and_p, rank_shape=grid,
                       grid_size=float(np.prod(grid)))
    lap = torch.zeros((2,) + grid, dtype=torch.float64, device=device)
    decomp.share_halos(f_arr)
    derivs(fx=f_arr, lap=lap)
    energy = red(f=f_arr, dfdt=dfdt_arr, lap_f=lap, a=np.ones(1))
    expand = ps.Expansion(energy["total"], ps.LowStorageRK54)
    for s in range(stepper.num_stages):
        stepper(s, a=expand.a, hubble=expand.hubble,
                f=f_arr, dfdt=dfdt_arr, lap_f=lap)
        expand.step(s, energy["total"], energy["pressure"], dt)
        decomp.share_halos(f_arr)
        derivs(fx=f_arr, lap=lap)
        energy = red(f=f_arr, dfdt=dfdt_arr, lap_f=lap, a=expand.a)
    print("4. one RK54 step: a =", float(expand.a[0]),
          "E =", energy["total"])

    # -- 5. Fourier stack ----------------------------------------------
    fft = ps.DFT(decomp, grid_shape=grid, dtype=np.float64,
                 device=device)
    spectra = ps.PowerSpectra(decomp, fft, dk, L ** 3)
    proj = ps.Projector(fft, h, dk, dx)
    gen = ps.RayleighGenerator(fft=fft, dk=dk, volume=L ** 3, seed=42)
    fld = torch.zeros(pad, dtype=torch.float64, device=device)
    gen.init_field(fld)
    spec = spectra(fld)
    print("5. Rayleigh field spectrum bins:", spec.shape,
          "peak bin:", int(np.argmax(spec)))
    hij_k = (torch.randn((6,) + tuple(fft.shape(True)),
                         dtype=torch.float64, device=device)
             + 0j).to(fft.fk.dtype)
    proj.transverse_traceless(hij_k)
    tr = (hij_k[0] + hij_k[3] + hij_k[5]).abs().max()
    print("5b. TT projection trace residual:", float(tr))
    # a user-written k-space map: a Gaussian filter, in place between
    # the transforms
    from pystella_amd.field import exp
    fk_ = Field("fk")
    kx, ky, kz = (Field(n, indices=(ix,))
                  for n, ix in (("kx", "i"), ("ky", "j"), ("kz", "k")))
    smooth = ps.KSpaceMap(
        {fk_: fk_ * exp(-(kx**2 + ky**2 + kz**2) * ps.var("s"))})
    before = float(fld.var())
    modes = fft.dft(fld)
    smooth(fk=modes, s=0.5 * (2 * dx[0] * dk[0])**2,
           kx=fft.sub_k["momenta_x"], ky=fft.sub_k["momenta_y"],
           kz=fft.sub_k["momenta_z"])
    fft.idft(modes, fld)
    print("5c. Gaussian-filtered field variance:", before, "->",
          float(fld.var()))

    # -- 6. multigrid ---------------------------------------------------
    from pystella_amd.derivs import _LAP_COEFS, centered_diff
    from pystella_amd.multigrid import (FullApproximationScheme,
                                        NewtonIterator, v_cycle)
    fb = Field("f", offset="h")
    rb = Field("rho", offset="h")
    lhs = sum(centered_diff(fb, _LAP_COEFS[1], direction=mu, order=2)
              for mu in range(1, 4)) / ps.var("dx") ** 2
    d1 = ps.DomainDecomposition((1, 1, 1), 1, rank_shape=grid)
    solver = NewtonIterator(d1, {fb: (lhs, rb)}, halo_shape=1,
                            fixed_parameters=dict(omega=0.8))
    mg = FullApproximationScheme(solver, halo_shape=1)
    pad1 = tuple(m + 2 for m in grid)
    rho_t = torch.zeros(pad1, dtype=torch.float64, device=device)
    rho_t[1:-1, 1:-1, 1:-1] = torch.rand(grid, device=device) - 0.5
    d1.share_halos(rho_t)
    ff2 = torch.zeros(pad1, dtype=torch.float64, device=device)
    errs = mg(d1, dx0=dx[0], cycle=v_cycle(4, 8, 1), f=ff2, rho=rho_t)
    first = [e for lvl, e in errs if lvl == 0][0]["f"][1]
    last = [e for lvl, e in errs if lvl == 0][-1]["f"][1]
    print("6. MG V-cycle residual:", first, "->", last)

    # -- 7. the fused hot loop -----------------------------------------
    from pystella_amd.fusion import (DeviceFriedmannLoop,
                                     StencilRKStepper)
    fst = StencilRKStepper(ps.LowStorageRK54, [sector], derivs,
                           halo_shape=h, rank_shape=grid, dt=dt,
                           reducers=sector,
                           grid_size=float(np.prod(grid)),
                           callback=get_rho_and_p)
    arrays = {"f": f_arr, "dfdt": dfdt_arr,
              "f_next": torch.zeros_like(f_arr)}
    if device.type == "cuda":
        loop = DeviceFriedmannLoop(fst, decomp, expand,
                                   float(np.prod(grid)), dt)
        loop.step(arrays)
        print("7. device loop state:", loop.read_state())
    else:
        en = None
        for s in range(fst.num_stages):
            en = fst(s, a=expand.a, hubble=expand.hubble, **arrays)
            for name in fst.pingpong:
                arrays[name], arrays[f"{name}_next"] = \
                    arrays[f"{name}_next"], arrays[name]
                decomp.share_halos(arrays[name])
            expand.step(s, en["total"], en["pressure"], dt)
        print("7. fused host loop energy:", en["total"])

    # -- 8. output + checkpoint ----------------------------------------
    from pystella_amd.checkpoint import load_checkpoint, save_checkpoint
    out = ps.OutputFile(name="tutorial_out")
    out.output("energy", t=0.0, total=float(np.asarray(
        energy["total"]).reshape(-1)[0]))
    out.close()
    save_checkpoint("tutorial_ckpt.h5", decomp,
                    {"f": arrays["f"]}, attrs={"t": dt})
    f_back = torch.zeros_like(arrays["f"])
    attrs = load_checkpoint("tutorial_ckpt.h5", decomp, {"f": f_back})
    # compare interiors: the device loop leaves halos stale by design
    # (they are refreshed lazily at the next stage's exchange), while
    # the checkpoint restore re-shares them
    cut = (slice(None),) + (slice(h, -h),) * 3
    assert torch.equal(f_back[cut], arrays["f"][cut])
    print("8. wrote", out.filename, "and tutorial_ckpt.h5; restored",
          "t =", attrs["t"])
    print("tutorial complete")
    return energy


if __name__ == "__main__":
    main()

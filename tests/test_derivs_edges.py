"""The AOT derivative kernels (csrc/derivs.hip) at a shape where no
tile is full, against the float64 numpy stencil of
tests/preheat_reference.py.

Grid (40, 11, 70) with the default x-chunk of 32 gives x-chunks of 32
and 8 (the ring is re-initialised at i0 != 0); for the LDS kernel
(32z x 8y tiles) three z-blocks with 6 live lanes in the last and two
y-blocks with 3 live rows in the last, so the clamped staging and the
inactive-but-staging lanes all occur; for the plain kernels (64z x 4y)
two z-blocks and three y-blocks, both with a short last block.
PYSTELLA_LDS=0 selects the plain-L1 gradlap_knl, the documented
fallback.  Outputs are NaN-filled before every call so an unwritten
site fails.
"""

import numpy as np
import pytest
import torch

import pystella_amd as ps
from tests.preheat_reference import fd_reference

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")

GRID = (40, 11, 70)
NF = 2
DX = (0.1, 0.11, 0.12)


def _padded_input(outer, h, tdtype, seed):
    """torch.rand padded input whose halos hold the periodic images of
    the interior (what share_halos writes on a single rank)."""
    torch.manual_seed(seed)
    pad = tuple(n + 2 * h for n in GRID)
    f = torch.rand(outer + pad, dtype=tdtype).numpy()
    cut = (slice(None),) * len(outer) + (slice(h, -h),) * 3
    width = ((0, 0),) * len(outer) + ((h, h),) * 3
    return torch.from_numpy(np.pad(f[cut], width, mode="wrap"))


def _run_case(monkeypatch, h, tdtype, lds, xchunk=None):
    for name, value in (("PYSTELLA_LDS", lds), ("PYSTELLA_XCHUNK", xchunk)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=GRID)
    derivs = ps.FiniteDifferencer(decomp, h, DX, rank_shape=GRID)
    tol = 1e-12 if tdtype == torch.float64 else 2e-4

    f = _padded_input((NF,), h, tdtype, seed=7)
    # fp32 reference: the float64 stencil of the same float32 inputs
    lap_r, pdx_r, pdy_r, pdz_r = fd_reference(f.numpy(), h, DX)
    grd_r = np.stack([pdx_r, pdy_r, pdz_r], axis=1)
    fg = f.cuda()

    def nans(*shape):
        return torch.full(shape + GRID, float("nan"), dtype=tdtype,
                          device="cuda")

    def check(what, got, ref):
        got = got.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any(), \
            f"{what}: {int(np.isnan(got).sum())} unwritten sites"
        err = np.abs(got - ref).max()
        bound = tol * (1. + np.abs(ref).max())
        print(f"    {what}: err {err:.3e}  bound {bound:.3e}")
        assert err < bound, (what, err, bound)

    # gradlap<LAP, GRAD>
    lap, grd = nans(NF), nans(NF, 3)
    derivs(fx=fg, lap=lap, grd=grd)
    check("lap (lap+grd)", lap, lap_r)
    check("grd (lap+grd)", grd, grd_r)
    # gradlap<LAP, -->
    lap = nans(NF)
    derivs(fx=fg, lap=lap)
    check("lap alone", lap, lap_r)
    # gradlap<--, GRAD>
    grd = nans(NF, 3)
    derivs(fx=fg, grd=grd)
    check("grd alone", grd, grd_r)
    # pd_knl, one axis at a time
    for name, ref in (("pdx", pdx_r), ("pdy", pdy_r), ("pdz", pdz_r)):
        out = nans(NF)
        derivs(fx=fg, **{name: out})
        check(name, out, ref)
    # the halo fill left the input alone
    assert torch.equal(fg.cpu(), f)

    # divergence: pd_knl then two accumulating pd_knl
    vec = _padded_input((3,), h, tdtype, seed=8)
    div_r = sum(fd_reference(vec[mu].numpy(), h, DX)[1 + mu]
                for mu in range(3))
    div = torch.full(GRID, float("nan"), dtype=tdtype, device="cuda")
    derivs.divergence(vec=vec.cuda(), div=div)
    check("divergence", div, div_r)
    torch.cuda.synchronize()


@requires_gpu
@pytest.mark.parametrize("lds", [None, "0"], ids=["lds", "plain"])
@pytest.mark.parametrize("tdtype", [torch.float64, torch.float32],
                         ids=["fp64", "fp32"])
@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_derivs_partial_tiles(h, tdtype, lds, monkeypatch):
    _run_case(monkeypatch, h, tdtype, lds)


@requires_gpu
@pytest.mark.parametrize("lds", [None, "0"], ids=["lds", "plain"])
def test_derivs_many_short_chunks(lds, monkeypatch):
    """PYSTELLA_XCHUNK=7: six x-chunks with a 5-long tail."""
    _run_case(monkeypatch, 2, torch.float64, lds, xchunk="7")

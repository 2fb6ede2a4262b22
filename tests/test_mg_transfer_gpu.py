"""The fused multigrid transfer kernels on a GPU (backend/hip.py
``mg_restrict`` / ``mg_interpolate``, routed from
multigrid/transfer.py): every operator against a direct, non-separable
float64 sum written here; what the kernels may and may not touch; which
calls take them; and a FAS solve with and without them.
"""

import itertools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.field import Field, shift_fields, var
from pystella_amd.multigrid import (
    FullApproximationScheme, RedBlackIterator, v_cycle)
from pystella_amd.multigrid.transfer import (
    CubicInterpolation, FullWeighting, Injection, LinearInterpolation)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

# -- the oracle: the operators' definitions, written out term by term

# restriction: {fine offset: coefficient} per axis
RESTRICTIONS = {
    "full_weighting": {-1: 0.25, 0: 0.5, 1: 0.25},
    "injection": {0: 1.0},
}
# prolongation: per axis, fine site 2i + p takes Σ_a c_a coarse[i + (p+a)//2]
PROLONGATIONS = {
    "linear": ({0: 1.0}, {-1: 0.5, 1: 0.5}),
    "cubic": ({0: 1.0}, {-3: -0.0625, -1: 0.5625, 1: 0.5625, 3: -0.0625}),
}
# number of terms of the largest sum of each operator
TERMS = {"full_weighting": 27, "injection": 1, "linear": 8, "cubic": 64}
MAKE = {"full_weighting": FullWeighting, "injection": Injection,
        "linear": LinearInterpolation, "cubic": CubicInterpolation}


def restrict_sum(fine, n2, h, coefs):
    """Σ_abc c_a c_b c_c fine[h+2i+a, h+2j+b, h+2k+c] over the coarse
    interior ``n2``, in float64, one term after the other."""
    out = np.zeros(fine.shape[:-3] + tuple(n2))
    for (a, ca), (b, cb), (c, cc) in itertools.product(coefs.items(),
                                                       repeat=3):
        out += (ca * cb * cc) * fine[
            ..., h + a:h + a + 2 * n2[0]:2, h + b:h + b + 2 * n2[1]:2,
            h + c:h + c + 2 * n2[2]:2]
    return out


def prolong_sum(coarse, n2, h, even, odd):
    """The fine interior ``2 n2`` of the tensor-product prolongation of
    ``coarse``, in float64: 8 parities, each a direct sum."""
    out = np.zeros(coarse.shape[:-3] + tuple(2 * n for n in n2))
    for px, py, pz in itertools.product((0, 1), repeat=3):
        acc = np.zeros(coarse.shape[:-3] + tuple(n2))
        cs = [(odd if p else even).items() for p in (px, py, pz)]
        for (a, ca), (b, cb), (c, cc) in itertools.product(*cs):
            oa, ob, oc = (px + a) // 2, (py + b) // 2, (pz + c) // 2
            acc += (ca * cb * cc) * coarse[
                ..., h + oa:h + oa + n2[0], h + ob:h + ob + n2[1],
                h + oc:h + oc + n2[2]]
        out[..., px::2, py::2, pz::2] = acc
    return out


def absolute(coefs):
    return {a: abs(c) for a, c in coefs.items()}


def oracle(op, f1, f2, n2, h, correct):
    """(want, mag) on the interior of the output, from the float64
    copies ``f1`` (fine) and ``f2`` (coarse) of the stored inputs."""
    if op in RESTRICTIONS:
        coefs = RESTRICTIONS[op]
        val = restrict_sum(f1, n2, h, coefs)
        mag = restrict_sum(np.abs(f1), n2, h, absolute(coefs))
        old = f2[(Ellipsis,) + tuple(slice(h, h + n) for n in n2)]
        sign = -1.0
    else:
        even, odd = PROLONGATIONS[op]
        val = prolong_sum(f2, n2, h, even, odd)
        mag = prolong_sum(np.abs(f2), n2, h, absolute(even), absolute(odd))
        old = f1[(Ellipsis,) + tuple(slice(h, h + 2 * n) for n in n2)]
        sign = 1.0
    if correct:
        return old + sign * val, np.abs(old) + mag
    return val, mag


# -- the cases

SHAPES = [(5, 3, 70), (4, 6, 8)]
OUTERS = [(), (3,)]
DTYPES = [torch.float32, torch.float64]
U_STORE = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}
CASES = [(op, h) for h in (1, 2)
         for op in ("full_weighting", "injection", "linear")] + [("cubic", 2)]


def sentinel_halo(shape, interior, dtype, rng, fill):
    """A padded array whose halo holds a different finite value at every
    site and whose interior is ``fill`` (None: standard normal)."""
    arr = 1000.0 + np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
    inner = (Ellipsis,) + interior
    arr[inner] = (rng.standard_normal(arr[inner].shape) if fill is None
                  else fill)
    return torch.from_numpy(arr).to(dtype)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("correct", [False, True], ids=["store", "correct"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("outer", OUTERS, ids=["scalar", "outer3"])
@pytest.mark.parametrize("n2", SHAPES, ids=["5x3x70", "4x6x8"])
@pytest.mark.parametrize("op,h", CASES,
                         ids=[f"{op}-h{h}" for op, h in CASES])
def test_operator_against_direct_sum(op, h, n2, outer, dtype, correct,
                                     monkeypatch):
    monkeypatch.delenv("PYSTELLA_MG_TRANSFER", raising=False)
    rng = np.random.default_rng(
        [CASES.index((op, h)), SHAPES.index(n2), len(outer), int(correct)])
    fine = outer + tuple(2 * n + 2 * h for n in n2)
    coarse = outer + tuple(n + 2 * h for n in n2)
    fine_in = tuple(slice(h, h + 2 * n) for n in n2)
    coarse_in = tuple(slice(h, h + n) for n in n2)
    restriction = op in RESTRICTIONS
    if restriction:
        f1 = torch.from_numpy(rng.standard_normal(fine)).to(dtype)
        f2 = sentinel_halo(coarse, coarse_in, dtype, rng,
                           None if correct else np.nan)
        src, out, out_in = f1, f2, coarse_in
    else:
        f2 = torch.from_numpy(rng.standard_normal(coarse)).to(dtype)
        f1 = sentinel_halo(fine, fine_in, dtype, rng,
                           None if correct else np.nan)
        src, out, out_in = f2, f1, fine_in
    want, mag = oracle(op, f1.double().numpy(), f2.double().numpy(), n2, h,
                       correct)

    d1, d2 = f1.cuda(), f2.cuda()
    calls = []
    name = "mg_restrict" if restriction else "mg_interpolate"
    kernel = getattr(hip, name)
    monkeypatch.setattr(hip, name,
                        lambda *a: (calls.append(a), kernel(*a))[1])
    ret = MAKE[op](halo_shape=h, correct=correct)(f1=d1, f2=d2)
    torch.cuda.synchronize()
    assert len(calls) == 1
    d_src, d_out = (d1, d2) if restriction else (d2, d1)
    assert ret is d_out

    # the input is untouched, bit for bit
    assert torch.equal(bits(d_src.cpu()), bits(src))
    got_all = d_out.cpu()
    # so is the output's halo
    inner = (Ellipsis,) + out_in
    halo = torch.ones(out.shape, dtype=torch.bool)
    halo[inner] = False
    assert torch.equal(bits(got_all)[halo], bits(out)[halo])
    # and the interior is the direct sum, rounded once
    got = got_all[inner].double().numpy()
    assert np.isfinite(got).all()
    bound = U_STORE[dtype] * np.abs(want) + 16 * TERMS[op] * 2.0**-53 * mag
    excess = np.abs(got - want) / bound
    print(f"{op} h={h} n2={n2} outer={outer} {dtype} correct={correct}: "
          f"max |got - want| / bound = {excess.max():.3g}")
    assert (np.abs(got - want) <= bound).all(), excess.max()


def test_empty_coarse_interior_makes_no_launch(monkeypatch):
    monkeypatch.delenv("PYSTELLA_MG_TRANSFER", raising=False)
    launches = []
    ext = hip.ext()

    class Spy:
        def __getattr__(self, name):
            if name == "jit_launch":
                return lambda *a: launches.append(a)
            return getattr(ext, name)

    h = 1
    f1 = torch.full((2, 10 + 2 * h, 2 * h, 6 + 2 * h), 7.0, device="cuda")
    f2 = torch.full((2, 5 + 2 * h, 2 * h, 3 + 2 * h), 5.0, device="cuda")
    monkeypatch.setattr(hip, "ext", lambda: Spy())
    FullWeighting(h)(f1=f1, f2=f2)
    LinearInterpolation(h, correct=True)(f1=f1, f2=f2)
    assert launches == []
    assert (f1 == 7.0).all() and (f2 == 5.0).all()


# -- routing

def _pair(h, n2=(3, 4, 5), dtype=torch.float32, seed=3):
    gen = torch.Generator().manual_seed(seed)
    f1 = torch.randn(tuple(2 * n + 2 * h for n in n2), dtype=dtype,
                     generator=gen).cuda()
    f2 = torch.randn(tuple(n + 2 * h for n in n2), dtype=dtype,
                     generator=gen).cuda()
    return f1, f2


def _strided(f1, f2):
    wide = torch.zeros(f1.shape[:-1] + (f1.shape[-1] + 1,), dtype=f1.dtype,
                       device=f1.device)
    wide[..., :-1] = f1
    return wide[..., :-1], f2


def _mixed(f1, f2):
    return f1, f2.double()


def _too_long(f1, f2):
    return torch.cat([f1, f1[..., :1]], dim=-1).contiguous(), f2


def _overlapping(f1, f2):
    buf = torch.cat([f1.reshape(-1), f2.reshape(-1)])
    start = f1.numel() - 7
    return (buf[:f1.numel()].view(f1.shape),
            buf[start:start + f2.numel()].view(f2.shape))


INELIGIBLE = {"strided": _strided, "mixed_dtypes": _mixed,
              "fine_too_long": _too_long, "overlapping": _overlapping}
OPERATORS = {
    "restrict": lambda: FullWeighting(1),
    "restrict_and_correct": lambda: FullWeighting(1, correct=True),
    "interpolate": lambda: LinearInterpolation(1),
    "interpolate_and_correct": lambda: LinearInterpolation(1, correct=True),
}


@pytest.fixture
def spies(monkeypatch):
    counts = {"mg_restrict": 0, "mg_interpolate": 0}

    def spy(name):
        kernel = getattr(hip, name)

        def call(*args):
            counts[name] += 1
            return kernel(*args)
        return call
    for name in counts:
        monkeypatch.setattr(hip, name, spy(name))
    return counts


@pytest.mark.parametrize("which", OPERATORS)
def test_eligible_call_is_one_launch_and_the_knob_turns_it_off(
        which, spies, monkeypatch):
    monkeypatch.delenv("PYSTELLA_MG_TRANSFER", raising=False)
    op = OPERATORS[which]()
    name = "mg_restrict" if "restrict" in which else "mg_interpolate"
    op(f1=_pair(1)[0], f2=_pair(1)[1])
    assert spies[name] == 1 and sum(spies.values()) == 1
    op(None, *_pair(1))
    assert spies[name] == 2 and sum(spies.values()) == 2
    monkeypatch.setenv("PYSTELLA_MG_TRANSFER", "0")
    op(f1=_pair(1)[0], f2=_pair(1)[1])
    assert sum(spies.values()) == 2
    monkeypatch.setenv("PYSTELLA_MG_TRANSFER", "1")
    op(f1=_pair(1)[0], f2=_pair(1)[1])
    assert spies[name] == 3


@pytest.mark.parametrize("case", INELIGIBLE)
@pytest.mark.parametrize("which", OPERATORS)
def test_ineligible_call_runs_the_torch_form(which, case, spies,
                                             monkeypatch):
    op = OPERATORS[which]()
    monkeypatch.delenv("PYSTELLA_MG_TRANSFER", raising=False)
    f1, f2 = INELIGIBLE[case](*_pair(1))
    ret = op(f1=f1, f2=f2)
    assert sum(spies.values()) == 0
    monkeypatch.setenv("PYSTELLA_MG_TRANSFER", "0")
    g1, g2 = INELIGIBLE[case](*_pair(1))
    want = op(f1=g1, f2=g2)
    assert sum(spies.values()) == 0
    assert ret is (f2 if "restrict" in which else f1)
    assert torch.equal(ret, want)
    assert torch.equal(f1, g1) and torch.equal(f2, g2)


def test_cubic_at_halo_one_is_refused_as_before():
    with pytest.raises(ValueError):
        CubicInterpolation(1)


# -- memory

@pytest.mark.parametrize("which", OPERATORS)
def test_fused_call_allocates_nothing(which, monkeypatch):
    monkeypatch.delenv("PYSTELLA_MG_TRANSFER", raising=False)
    op = OPERATORS[which]()
    f1, f2 = _pair(1, n2=(16, 16, 64))
    op(f1=f1, f2=f2)            # compiles
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    assert torch.cuda.max_memory_allocated() == base
    op(f1=f1, f2=f2)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base
    # where the torch form does allocate
    monkeypatch.setenv("PYSTELLA_MG_TRANSFER", "0")
    op(f1=f1, f2=f2)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() > base


# -- end to end

RANK_SHAPE = (8, 12, 144)


def _fas(device, dtype):
    """Final f and last level-0 residual L2 norm of one V-cycle on the
    Poisson problem of ``test_multigrid_fas_gpu``."""
    h = 1
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=RANK_SHAPE)
    dx = (2 * np.pi / RANK_SHAPE[0],) * 3
    f = Field("f", offset="h")
    rho = Field("rho", offset="h")
    lap = sum(
        (shift_fields(f, tuple(s * int(m == d) for m in range(3)))
         - 2 * f
         + shift_fields(f, tuple(-s * int(m == d) for m in range(3))))
        for d in range(3) for s in [1]) / var("dx")[0]**2
    solver = RedBlackIterator(decomp, {f: (lap, rho)}, halo_shape=h,
                              fixed_parameters=dict(omega=1.0))
    mg = FullApproximationScheme(solver, halo_shape=h)
    # one period of a sine along each axis: a smooth, zero-mean source
    sins = [torch.sin(torch.arange(n, dtype=torch.float64) * (2 * np.pi / n))
            for n in RANK_SHAPE]
    f_exact = sins[0][:, None, None] * sins[1][None, :, None] * sins[2]
    pad = tuple(n + 2 * h for n in RANK_SHAPE)
    rho_t = torch.zeros(pad, dtype=torch.float64)
    rho_t[h:-h, h:-h, h:-h] = -3.0 * f_exact
    rho_t = rho_t.to(dtype).to(device)
    decomp.share_halos(rho_t)
    ff = torch.zeros(pad, dtype=dtype, device=device)
    errs = mg(decomp, dx0=dx, cycle=v_cycle(2, 2, 2), f=ff, rho=rho_t)
    resid = [e for lvl, e in errs if lvl == 0][-1]["f"][1]
    return ff[h:-h, h:-h, h:-h].double().cpu(), float(resid)


def _apart(a, b):
    """(largest difference of f relative to the largest |f|, relative
    difference of the residual norms) of two ``_fas`` results."""
    return ((a[0] - b[0]).abs().max().item() / b[0].abs().max().item(),
            abs(a[1] - b[1]) / abs(b[1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_fas_solve_fused_against_torch_transfers(dtype, spies, monkeypatch):
    """One V-cycle with the fused transfers lies no further from the
    same cycle with the torch transfers, both on the GPU, than four
    times the distance between the torch-transfer cycle on the GPU and
    on the CPU (which differ by contraction in the smoother kernels):
    the fused transfers perturb all four transfers by rounding, the
    reference pair only the smoother, and both are rounding-level
    changes to the same contractive iteration.  The spread is measured
    here, in the same run.

    Measured on an MI355X (f relative to the largest |f|, resid_L2
    relative): float32, torch GPU against torch CPU 1.18e-7 and 4.7e-7,
    fused against torch GPU 1.18e-7 and 4.15e-8.  float64, torch GPU
    against torch CPU 0 and 0, the two are equal to the bit, so the
    bound is zero; fused against torch GPU 0 and 0, because the kernels
    sum in the chain's order and full weighting's and linear
    interpolation's coefficients make every product exact, which leaves
    the float64 kernels no rounding that the chain does not make.
    """
    monkeypatch.setenv("PYSTELLA_MG_TRANSFER", "0")
    torch_cpu = _fas("cpu", dtype)
    torch_gpu = _fas("cuda", dtype)
    assert sum(spies.values()) == 0
    monkeypatch.delenv("PYSTELLA_MG_TRANSFER")
    fused = _fas("cuda", dtype)
    assert spies["mg_restrict"] > 0 and spies["mg_interpolate"] > 0
    spread = _apart(torch_gpu, torch_cpu)
    diff = _apart(fused, torch_gpu)
    print(f"{dtype}: torch GPU vs torch CPU: f {spread[0]:.3g}, "
          f"resid_L2 {spread[1]:.3g}; fused vs torch GPU: f {diff[0]:.3g}, "
          f"resid_L2 {diff[1]:.3g}")
    assert torch.isfinite(fused[0]).all() and fused[1] > 0
    assert diff[0] <= 4 * spread[0], (diff, spread)
    assert diff[1] <= 4 * spread[1], (diff, spread)

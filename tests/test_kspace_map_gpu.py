"""KSpaceMap on the GPU (backend/hip.py ``JitKspaceMap``): every case of
tests/kspace_map_reference.py against numpy at the derived tolerance and
against the CPU KSpaceMap, outputs NaN-filled between sentinel guards;
the spectral-derivatives case against the hand-written kernels; the
kernel cache; the refusals; and the routing of what existed before.

k-shape (12, 10, 8) is 960 modes, three full blocks of 256 and one of
192 threads; (5, 1, 3) is a single partial block with an extent of one.
"""

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.field import Field, var
from tests.kspace_map_reference import (
    CASES, KSHAPE, SMALL, assert_close, expected)
from tests.test_kspace_map_cpu import run_case

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

GUARD = 256
SENTINEL = 1234.5


class Guarded:
    """An output between two sentinel slabs, NaN before the call."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype,
                              device="cuda")
        self.out = self.buf[GUARD:GUARD + n].view(shape)
        self.out.fill_(float("nan"))
        assert self.out.is_contiguous()

    def guards_intact(self):
        n = self.out.numel()
        return bool((self.buf[:GUARD] == SENTINEL).all()
                    and (self.buf[GUARD + n:] == SENTINEL).all())


def _tdtype(npdtype):
    return torch.from_numpy(np.empty(0, npdtype)).dtype


def run_gpu(case, kshape, form, scalars=None, m=None):
    """Like ``run_case`` on the device, every output guarded (an output
    that is also an input holds the input)."""
    inputs = case.inputs(kshape, form)
    env, guarded = {}, {}
    for name, outer in case.outputs.items():
        guarded[name] = Guarded(tuple(outer) + tuple(kshape),
                                _tdtype(case.forms[form][name]))
        env[name] = guarded[name].out
    for name, a in inputs.items():
        t = torch.as_tensor(a, device="cuda")
        if name in env:
            env[name].copy_(t)
        else:
            env[name] = t
    before = {n: env[n].clone() for n in inputs if n not in case.outputs}
    m = m or ps.KSpaceMap(case.statements, case.tmp, name=case.name)
    m(**env, **(case.scalars if scalars is None else scalars))
    torch.cuda.synchronize()
    for name, g in guarded.items():
        assert g.guards_intact(), name
    for name, t in before.items():
        assert torch.equal(env[name], t), name
    return inputs, {n: env[n].cpu().numpy() for n in case.outputs}, m


def check(case, kshape, form, scalars=None, m=None):
    """The GPU result against numpy and against the CPU KSpaceMap."""
    inputs, got, m = run_gpu(case, kshape, form, scalars, m)
    _, cpu, _ = run_case(case, kshape, form, scalars=scalars)
    want = expected(case, inputs, scalars)
    for (name, comp), (w, mag, n) in want.items():
        what = f"{case.name}/{form} {name}[{comp}]"
        pick = (lambda x: x[name]) if comp is None \
            else (lambda x: x[name][comp])
        dtype = case.forms[form][name]
        assert_close(pick(got), w, mag, n, dtype, "gpu " + what)
        assert_close(pick(got), pick(cpu).astype(np.complex128), mag, n,
                     dtype, "gpu vs cpu " + what)
    for name, outer in case.outputs.items():
        for comp in range(outer[0] if outer else 0):
            if (name, comp) not in want:
                assert np.isnan(got[name][comp].real).all(), (name, comp)
    return inputs, got, m


@pytest.mark.parametrize("name,form", [
    ("derivs", "double"), ("derivs", "mixed"), ("phase", "double"),
    ("conj_div", "mixed"), ("vector", "double"), ("vector", "mixed"),
    ("mixed", "mixed")])
def test_case(name, form):
    check(CASES[name], KSHAPE, form)


@pytest.mark.parametrize("name,form", [("derivs", "double"),
                                       ("phase", "mixed")])
def test_degenerate_shape(name, form):
    check(CASES[name], SMALL, form)


@pytest.mark.parametrize("form", ["double", "mixed"])
def test_derivs_against_the_hand_written_kernel(form):
    """Equal bits are not demanded: the map's products may contract,
    the hand-written kernel shields its own."""
    case = CASES["derivs"]
    inputs, got, _ = run_gpu(case, KSHAPE, form)
    ctype = torch.complex128 if form == "double" else torch.complex64
    dev = {n: torch.as_tensor(a, device="cuda") for n, a in inputs.items()}
    outs = {n: torch.zeros(KSHAPE, dtype=ctype, device="cuda")
            for n in case.outputs}
    fn = hip.kspace_derivs if form == "double" else hip.kspace_derivs_c64
    fn(dev["fk"], outs, [dev[f"k1{a}"] for a in "xyz"],
       [dev[f"k2{a}"] for a in "xyz"], case.scalars["inv_n"])
    torch.cuda.synchronize()
    for (name, _), (w, mag, n) in expected(case, inputs).items():
        dtype = case.forms[form][name]
        hand = outs[name].cpu().numpy()
        assert_close(hand, w, mag, n, dtype, f"hand-written {name}")
        assert_close(got[name], hand.astype(np.complex128), mag, n, dtype,
                     f"map vs hand-written {name}")


def test_in_place_filter_compiles_once(monkeypatch):
    case = CASES["filter"]
    compiled = []
    native = hip.ext()

    class Spy:
        def __getattr__(self, attr):
            return getattr(native, attr)

        def jit_compile(self, src, name):
            compiled.append(name)
            return native.jit_compile(src, name)

    monkeypatch.setattr(hip, "ext", Spy)
    _, first, m = check(case, KSHAPE, "mixed")
    assert compiled == ["filter"] and len(m._kernels) == 1
    other = {"s": 0.008}
    _, second, _ = check(case, KSHAPE, "mixed", scalars=other, m=m)
    assert compiled == ["filter"] and len(m._kernels) == 1
    assert not np.array_equal(first["fk"], second["fk"])
    # another layout is another kernel
    check(case, KSHAPE, "double", m=m)
    assert compiled == ["filter", "filter"] and len(m._kernels) == 2


# -- refusals

class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"the native module's {name} was reached")


def _args():
    return {"fk": torch.ones(KSHAPE, dtype=torch.complex64, device="cuda"),
            "vk": torch.ones((3,) + KSHAPE, dtype=torch.complex128,
                             device="cuda"),
            "out": torch.ones(KSHAPE, dtype=torch.complex128,
                              device="cuda"),
            "kx": torch.ones(12, dtype=torch.float64, device="cuda")}


def test_refusals(monkeypatch):
    monkeypatch.setattr(hip, "ext", _NoLaunch)
    fk, out, vk = Field("fk"), Field("out"), Field("vk", shape=(3,))
    kx = Field("kx", indices=("i",))
    m = ps.KSpaceMap({out: fk * kx + vk[2]})
    a = _args()
    with pytest.raises(ValueError, match="out and vk overlap"):
        m(**{**a, "out": a["vk"][1]})
    flat = torch.ones(960 + 8, dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError, match="overlap in memory"):
        m(**{**a, "out": flat[8:].view(KSHAPE),
             "fk": flat[:960].view(KSHAPE)})
    with pytest.raises(TypeError, match="on one device.*kx on cpu"):
        m(**{**a, "kx": a["kx"].cpu()})
    strided = torch.ones((12, 10, 16), dtype=torch.complex64,
                         device="cuda")[:, :, ::2]
    with pytest.raises(ValueError, match="fk must be contiguous"):
        m(**{**a, "fk": strided})
    with pytest.raises(ValueError, match="argument kx has shape"):
        m(**{**a, "kx": a["kx"][:-1].contiguous()})
    with pytest.raises(ValueError, match="argument vk has shape"):
        m(**{**a, "vk": a["vk"][:2].contiguous()})
    with pytest.raises(TypeError, match="scalar s is complex"):
        ps.KSpaceMap({out: fk * var("s")})(fk=a["fk"], out=a["out"], s=1j)
    with pytest.raises(NotImplementedError, match="sqrt"):
        from pystella_amd.field import sqrt
        ps.KSpaceMap({out: sqrt(fk)})(fk=a["fk"], out=a["out"])
    # zero volume: nothing is compiled or launched
    shape = (4, 0, 3)
    m(fk=torch.ones(shape, dtype=torch.complex64, device="cuda"),
      vk=torch.ones((3,) + shape, dtype=torch.complex128, device="cuda"),
      out=torch.ones(shape, dtype=torch.complex128, device="cuda"),
      kx=torch.ones(4, dtype=torch.float64, device="cuda"))


# -- routing

def test_real_elementwise_map_takes_its_own_kernel(monkeypatch):
    calls = []
    real_get = hip.get_elementwise_kernel

    def counted(*args, **kwargs):
        calls.append("elementwise")
        return real_get(*args, **kwargs)

    def never(*args, **kwargs):
        raise AssertionError("an ElementWiseMap reached JitKspaceMap")

    monkeypatch.setattr(hip, "get_elementwise_kernel", counted)
    monkeypatch.setattr(hip, "JitKspaceMap", never)
    f, g = Field("f"), Field("g")
    m = ps.ElementWiseMap({g: 2 * f + var("a")})
    tf = torch.rand((6, 5, 4), dtype=torch.float64, device="cuda")
    tg = torch.zeros_like(tf)
    m(f=tf, g=tg, a=0.5)
    torch.cuda.synchronize()
    assert calls == ["elementwise"]
    assert torch.equal(tg, 2 * tf + 0.5)


def test_spectral_classes_reach_their_entry_points(monkeypatch):
    from tests.kspace_c64_reference import (
        GRID, class_inputs, make_collocator, make_solver)
    names = ("kspace_derivs", "kspace_div_accum", "kspace_poisson")
    names += tuple(n + "_c64" for n in names)
    counts = dict.fromkeys(names, 0)
    for name in names:
        def counted(*args, _name=name, _fn=getattr(hip, name), **kwargs):
            counts[_name] += 1
            return _fn(*args, **kwargs)
        monkeypatch.setattr(hip, name, counted)

    def never(*args, **kwargs):
        raise AssertionError("a spectral class reached JitKspaceMap")

    monkeypatch.setattr(hip, "JitKspaceMap", never)
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    # one transform dtype: the complex64 forms' routing is
    # tests/test_kspace_c64_gpu.py's
    fx, vec, rho = (t.cuda() for t in class_inputs("12x10x14"))
    coll = make_collocator("12x10x14", "cuda", np.float64)
    lap = torch.zeros_like(fx[0])
    grd = torch.zeros((3,) + GRID, dtype=torch.float64, device="cuda")
    coll(fx=fx[0], lap=lap, grd=grd)
    assert counts == {**dict.fromkeys(names, 0), "kspace_derivs": 1}
    div = torch.zeros(GRID, dtype=torch.float64, device="cuda")
    coll.divergence(vec=vec[0], div=div)
    assert counts["kspace_div_accum"] == 3
    solver = make_solver("12x10x14", "cuda", np.float64)
    solver(fx=lap, rho=rho, m_squared=1.7)
    torch.cuda.synchronize()
    assert counts == {**dict.fromkeys(names, 0), "kspace_derivs": 1,
                      "kspace_div_accum": 3, "kspace_poisson": 1}

"""The generated HIP source of KSpaceMap kernels (backend/hip.py
``JitKspaceMap``, backend/codegen.py ``KspaceCodegen``): produced with
``compile=False`` and inspected without a device, cross-compiled for
gfx950 where hipcc is present; and three existing real kernels, whose
source must not have moved.
"""

import hashlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.field import Field, get_field_args, var
from pystella_amd.field import expr as ex
from tests.kspace_map_reference import CASES, KSHAPE, SMALL

ELEM = {"complex128": "double2", "complex64": "float2", "float64": "double",
        "float32": "float"}
FORMS = [(name, form) for name in CASES for form in ("double", "mixed")]
IDS = [f"{n}-{f}" for n, f in FORMS]


def _dtypes(case, form):
    import numpy as np
    return {n: np.dtype(d).name for n, d in case.forms[form].items()}


def _source(name, form, kshape=KSHAPE):
    case = CASES[name]
    m = ps.KSpaceMap(case.statements, case.tmp, name=case.name)
    return m.source(kshape, _dtypes(case, form))


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _body(src):
    return src.split('extern "C"')[1]


@pytest.fixture
def no_native_module(monkeypatch):
    def no_ext():
        raise AssertionError("compile=False touched the native module")
    monkeypatch.setattr(hip, "ext", no_ext)


@pytest.mark.parametrize("name,form", FORMS, ids=IDS)
def test_source(name, form, no_native_module):
    case = CASES[name]
    src = _source(name, form)
    dtypes = _dtypes(case, form)
    assert "#define NKX 12\n#define NKY 10\n#define NKZ 8\n" in src
    body = _body(src)
    assert "const long idx = (long)blockIdx.x * 256 + threadIdx.x;" in body
    assert "if (idx >= VOLK) return;" in body
    assert "__launch_bounds__(256)" in body
    # pointers, by name, typed by the argument's dtype; a stored one
    # carries neither const nor __restrict__
    params = _params(src, case.name)
    ptrs = [p for p in params if "*" in p]
    assert [p.split()[-1] for p in ptrs] == sorted(dtypes)
    for p in ptrs:
        arg = p.split()[-1]
        if arg in case.outputs:
            assert p == f"{ELEM[dtypes[arg]]}* {arg}", p
        else:
            assert p == f"const {ELEM[dtypes[arg]]}* __restrict__ {arg}", p
    scalars = [p for p in params if "*" not in p]
    assert scalars == [f"const double s_{s}" for s in case.scalars]
    # one store statement per output component, each rounding once
    stores = re.findall(r"^\s*(\w+)\[(.*?)\] = (.*);$", body, re.M)
    assert len(stores) == len(case.statements)
    for (arg, off, rhs), lhs in zip(stores, case.statements):
        assert arg == lhs.name
        comp = int(lhs.index[0]) if hasattr(lhs, "index") else 0
        assert off == (f"{comp}L*VOLK + idx" if comp else "idx")
        elem = ELEM[dtypes[arg]]
        assert re.fullmatch(
            r"make_%s\(\(%s\)o(\d+)\.x, \(%s\)o\1\.y\)"
            % (elem, elem[:-1], elem[:-1]), rhs), rhs
    # one load per value read, all through the widening ps_load
    loads = re.findall(r"ps_load\((\w+) \+ \((.*?)\)\);", body)
    assert len(loads) == len(set(loads))
    assert "float" not in body.replace("make_float2", "").replace(
        "(float)", "").replace("float2*", "").replace("float*", "")


@pytest.mark.parametrize("kshape,lin32", [(KSHAPE, True), (SMALL, True),
                                          ((2048, 2048, 1025), False)])
def test_index_decode(kshape, lin32, no_native_module):
    """Emitted only for a map with axis fields; 32-bit below 2^31
    modes."""
    src = _source("conj_div", "mixed", kshape)
    for word in ("ii", "jj", "kk", "lin"):
        assert not re.search(r"\b%s\b" % word, _body(src)), word
    src = _source("filter", "mixed", kshape)
    body = _body(src)
    assert ("const unsigned lin = (unsigned)idx;" in body) == lin32
    assert ("const int kk = (int)(idx % NKZ);" in body) == (not lin32)
    for tab, ix in (("kx", "ii"), ("ky", "jj"), ("kz", "kk")):
        assert f"ps_load({tab} + ({ix}))" in body


def test_source_only_kernel(no_native_module):
    case = CASES["phase"]
    dtypes = _dtypes(case, "mixed")
    args = get_field_args({**case.tmp, **case.statements})

    def kernel(dtypes):
        return hip.JitKspaceMap(case.statements, case.tmp, args, dtypes,
                                KSHAPE, name=case.name, compile=False)

    k = kernel(dtypes)
    assert k.key is None and k.source == _source("phase", "mixed")
    # torch dtypes or their names
    assert k.source == kernel({n: getattr(torch, d)
                               for n, d in dtypes.items()}).source
    assert "ps_cexp(ps_times_i(1.0, " in k.source
    with pytest.raises(RuntimeError, match="compile=False"):
        k({})
    with pytest.raises(TypeError, match="fk has dtype torch.int32"):
        kernel({**dtypes, "fk": torch.int32})
    with pytest.raises(TypeError, match="axis table kx"):
        kernel({**dtypes, "kx": "complex128"})


def test_a_stored_component_is_loaded_again(no_native_module):
    a, b = Field("a"), Field("b", shape=(2,))
    m = ps.KSpaceMap({b[0]: a + b[1], b[1]: a * b[0], a: b[1] + b[0]})
    body = _body(m.source(KSHAPE, {"a": "complex64", "b": "complex128"}))
    assert len(re.findall(r"ps_load\(a \+", body)) == 1
    assert len(re.findall(r"ps_load\(b \+ \(idx\)\)", body)) == 1
    assert len(re.findall(r"ps_load\(b \+ \(1L\*VOLK \+ idx\)\)", body)) == 2
    # in order: the reload follows the store it must see
    assert body.index("b[idx] = ") < body.index("ps_load(b + (idx))")


# -- existing real kernels: sha256 of their generated source, taken
# before KspaceCodegen existed

SHA256_BEFORE = {
    "elementwise":
        "f28d49cf3fcf641ff64c087199c90de55d875bbbeb68043dc4d9feb10367fe88",
    "reduction":
        "852f13eecd24034bcd3ca1bdbcfd0162590ba3601d0ee0cf8b365cd13f101d61",
    "stage_float32":
        "7f0828bf06661f792643f3a509f882f9348d941c4bb5075bb335c083dc49b373",
}


class _SourceOnly:
    """Stands in for the native module: records what would compile."""

    def __init__(self):
        self.sources = []

    def jit_compile(self, src, name):
        self.sources.append(src)
        return name


def _existing_sources(monkeypatch):
    f, g = Field("f", offset="h", shape=(2,)), Field("g")
    a = var("a")
    stmts = {g: a * f[0]**2 + ex.exp(-f[1]) / (1 + ex.fabs(f[0]))}
    args = get_field_args(stmts)
    fake = _SourceOnly()
    monkeypatch.setattr(hip, "ext", lambda: fake)
    ew = hip.JitElementwise(stmts, {}, args, ["a"], (2, 2, 2), (12, 10, 8))
    red = hip.JitReduction([(a * f[0] * f[1], "sum"), (f[1]**3, "max")],
                           get_field_args([f]), ["a"], (2, 2, 2),
                           (12, 10, 8), dtype=torch.float32)
    assert fake.sources == [ew.source, red.source]
    from tests.test_stage_fp32_source import stage_kernel
    return {"elementwise": ew.source, "reduction": red.source,
            "stage_float32": stage_kernel(1, "float32", True).source}


def test_existing_real_kernels_have_not_moved(monkeypatch):
    for name, src in _existing_sources(monkeypatch).items():
        assert "cplx" not in src, name
        assert hashlib.sha256(src.encode()).hexdigest() \
            == SHA256_BEFORE[name], name


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_sources_compile_for_gfx950(tmp_path):
    """Device-only cross-compilation of every case's source, to
    assembly: no scratch, at most 64 VGPRs (eight waves per SIMD), a
    complex128 mode one 16-byte access and a complex64 mode one of 8."""
    procs = []
    for name, form in FORMS:
        path = tmp_path / f"{name}_{form}.hip"
        path.write_text(_source(name, form))
        procs.append((name, form, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-std=c++17", "-ffp-contract=fast",
             "-include", "hip/hip_runtime.h",
             "-S", str(path), "-o", str(tmp_path / f"{name}_{form}.s")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for name, form, proc in procs:
        ident = f"{name}-{form}"
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (ident, out[-3000:])
        asm = (tmp_path / f"{name}_{form}.s").read_text()
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", asm), ident
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", asm).group(1))
        sgprs = int(re.search(r"\.sgpr_count:\s+(\d+)", asm).group(1))
        print(f"{ident}: {vgprs} VGPRs, {sgprs} SGPRs")
        assert vgprs <= 64, (ident, vgprs)
        code = asm[:asm.index("s_endpgm")]
        ops = re.findall(r"^\s*(global_(?:load|store)_\w+)", code, re.M)
        case = CASES[name]
        dtypes = _dtypes(case, form)
        # stores: one per statement, of the target's width
        width = {"complex128": "dwordx4", "complex64": "dwordx2",
                 "float64": "dwordx2", "float32": "dword"}
        want_stores = sorted(f"global_store_{width[dtypes[lhs.name]]}"
                             for lhs in case.statements)
        assert sorted(o for o in ops if "store" in o) == want_stores, \
            (ident, ops)
        # loads: every grid value read is one access of its width
        body = _body(_source(name, form))
        want_loads = sorted(
            f"global_load_{width[dtypes[arg]]}"
            for arg, off in re.findall(r"ps_load\((\w+) \+ \((.*?)\)\);",
                                       body))
        assert sorted(o for o in ops if "load" in o) == want_loads, \
            (ident, ops)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_every_overload_compiles_for_gfx950(tmp_path):
    """What the cases leave out: integer powers of a complex value (the
    ps_powN templates on ``cplx``), a reciprocal, a general complex
    literal, every real/complex operand order, a promoted conditional
    and a real output."""
    a, b, w = Field("a"), Field("b"), Field("w")
    o, r = Field("o"), Field("r")
    t = var("t")
    m = ps.KSpaceMap(
        {o: a**3 + a**-2 + (2 + 3j) * ex.conj(b) + t / a + a / t + (t - a)
            + (a - t) - a / b + 1 / b + ex.If(w > 0, a, 2.5),
         r: ex.abs(a) + ex.real(b)**2 - ex.imag(a * b) + abs(w)
            + ex.exp(w) + ex.conj(w) + ex.imag(w)},
        {t: w * var("s") + 1})
    src = m.source(KSHAPE, {"a": "complex128", "b": "complex64",
                            "w": "float32", "o": "complex64",
                            "r": "float32"})
    assert "ps_pow3(v" in src and "(1.0/ps_pow2(v" in src
    assert "cplx(2.0, 3.0)" in src and "const double t = " in src
    path = tmp_path / "overloads.hip"
    path.write_text(src)
    proc = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
         "-std=c++17", "-ffp-contract=fast", "-include",
         "hip/hip_runtime.h", "-S", str(path), "-o",
         str(tmp_path / "overloads.s")],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
        timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:]
    asm = (tmp_path / "overloads.s").read_text()
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", asm)
    code = asm[:asm.index("s_endpgm")]
    stores = re.findall(r"^\s*(global_store_\w+)", code, re.M)
    assert sorted(stores) == ["global_store_dword", "global_store_dwordx2"]

"""The complex64 forms of the fused k-space kernels (backend/hip.py
``kspace_source`` with ``ctype="complex64"``): every source generated
and inspected without a device and cross-compiled for gfx950 where hipcc
is present; and the complex128 forms, which must not change by a byte.
"""

import hashlib
import itertools
import os
import re
import shutil
import subprocess

import pytest
import torch

from pystella_amd.backend import hip

KSHAPE = (12, 10, 8)
OUTS = ("pdx", "pdy", "pdz", "lap")
MASKS = [m for r in range(1, 5) for m in itertools.combinations(OUTS, r)]

# (identifier, op, flags) of every form
FORMS = [("derivs:" + "+".join(m), "derivs", {"outs": m}) for m in MASKS]
FORMS += [(f"div_accum:{mu}:{int(acc)}", "div_accum",
           {"mu": mu, "accumulate": acc})
          for mu in range(3) for acc in (False, True)]
FORMS += [("poisson", "poisson", {})]
IDS = [f[0] for f in FORMS]

# sha256 of each complex128 source at KSHAPE, as kspace_source gave them
# before it took a ctype
SHA256_C128 = {
    "derivs:pdx":
        "e36a6859c9ae095539f9bd627d4f815252c821e04cabad4e142ac934d1850be9",
    "derivs:pdy":
        "ef28ebcfb88d74e5177aa72178581375566f56d4abb328ff968b5def693b8c33",
    "derivs:pdz":
        "b10dc8511a7afec0c0f3804191e50b667943bd3eaad5f461b0d14a8706309527",
    "derivs:lap":
        "bda3655da0e378c18e238796d1cc9b452f5f25d6f851ee666315f06865b3ce3a",
    "derivs:pdx+pdy":
        "f99410e8c437dd919c217e71a23a6f693666947fd08c5d263538311289f61838",
    "derivs:pdx+pdz":
        "da40d1af8c5d3f03256f95673d856acf4537debcaca3e5359b11f3f832baca58",
    "derivs:pdx+lap":
        "1236d5cae29944f17fa14f64f8580c7289dca5352a626c7973df55f4da0b5259",
    "derivs:pdy+pdz":
        "30c8792cff310dedb8bac81ea3787a9db54b12e1d37f766ec2b3be9c7a064f24",
    "derivs:pdy+lap":
        "e38541514f7f672ff6c7d6bbc9c078af341dbb9ca3eb402a08044dcc2c40ff74",
    "derivs:pdz+lap":
        "9f61822d6cde2329fd82ccff107ed4efafbe69271307b9cbdaf91796eeb188f6",
    "derivs:pdx+pdy+pdz":
        "f97081a632fdc20d8f54159b278e421e5b1d59a3ad4bd689140060f5e12b9b99",
    "derivs:pdx+pdy+lap":
        "2f6c7fbc477bfbfd1afcdd1b8e2cde184b4e12d7cf18b6c4c5c3953a588faa6c",
    "derivs:pdx+pdz+lap":
        "55de7a70ffbc7357405b03f432064fcbfef719665924a5ed346bb18623d2b97b",
    "derivs:pdy+pdz+lap":
        "4f67f8b6c00ba526607323a8cd04dedbd7b74c6bfbf3b9f150cd47e340d953df",
    "derivs:pdx+pdy+pdz+lap":
        "fe56c3833cd142d83cb3c7a913c1d930c0b353e3e75cef632e8b81654f9d08c7",
    "div_accum:0:0":
        "2b5b3e2ff908f035e8b227ccfb986ae11eb9d385176279389e6ca0b75d943422",
    "div_accum:0:1":
        "5d65259e81594fe3bb38665893c53e921575ce2c074f0447f0bdde0c2e770921",
    "div_accum:1:0":
        "7ca41e8edb322821c23325c10c8a1122e31c217bdf328f1cc5a08ed66047493a",
    "div_accum:1:1":
        "8cb5fdd41b18b63ec017c71ff099c115799234fddba0554a0b32e4222a956886",
    "div_accum:2:0":
        "37f98a9285004c464912bd290ba15d11d9878a5eb96557ed9f09f22452ee5c62",
    "div_accum:2:1":
        "724725273ef625d30f70dea41bc0f56fc975ae71253074a6428f573a35ea6a6a",
    "poisson":
        "2a46da46b8533af5fcb8b4524cd50f1dc7b84d6b8700e5e86e4d9923ed45c948",
}

WIDEN = ("const float2 {v}_s = {p}[idx];\n"
         "    const double2 {v} = make_double2((double){v}_s.x, "
         "(double){v}_s.y);")


def _params(src, name):
    m = re.search(r"void %s\(\s*(.*?)\)\s*\{" % re.escape(name), src, re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _body(src):
    return src.split('extern "C"')[1]


def _stores(src):
    """(pointer, right-hand side) of every store of a mode."""
    return re.findall(r"^\s*(\w+)\[idx\] = (.*);$", _body(src), re.M)


def _check_common(src, name, written):
    """What every complex64 source has; ``written`` are the outputs."""
    params = _params(src, name)
    modes = [p for p in params if "float2" in p]
    rest = [p for p in params if "float2" not in p]
    assert modes[0].startswith("const float2* ")
    assert [p.split()[-1] for p in modes[1:]] == list(written)
    assert all(p.startswith("float2* ") for p in modes[1:])
    # tables and scalars are double
    assert rest and all(p.startswith(("const double* __restrict__ ",
                                      "const double ")) for p in rest)
    assert "double2*" not in src
    # exactly one store per requested output, each one make_float2 of
    # two converted double expressions
    stores = _stores(src)
    assert [p for p, _ in stores] == list(written)
    for _, rhs in stores:
        assert re.fullmatch(
            r"make_float2\(\(float\)\(.+\), \(float\)\(.+\)\)", rhs), rhs
    # float appears nowhere else: no float arithmetic, and the only
    # float2 values are the loaded modes
    body = _body(src)
    assert len(re.findall(r"\bfloat\b", body)) == 2 * len(stores)
    assert len(re.findall(r"\(float\)\(", body)) == 2 * len(stores)
    loads = re.findall(r"const float2 (\w+)_s = (\w+)\[idx\];", body)
    assert len(re.findall(r"\bfloat2\b", body)) == len(modes) + len(loads)
    # one widening per loaded component
    for v, p in loads:
        assert WIDEN.format(v=v, p=p) in body
        assert len(re.findall(r"\b%s_s\b" % v, body)) == 3
    assert len(re.findall(r"\(double\)", body)) == 2 * len(loads)
    return loads


@pytest.mark.parametrize("mask", MASKS, ids="+".join)
def test_derivs_c64_source(mask):
    src = hip.kspace_source("derivs", KSHAPE, ctype="complex64", outs=mask)
    assert src == hip.kspace_source("derivs", KSHAPE, torch.complex64,
                                    outs=mask[::-1])
    assert "#define NKX 12\n#define NKY 10\n#define NKZ 8\n" in src
    assert "if (idx >= VOLK) return;" in src
    written = [o for o in OUTS if o in mask]
    loads = _check_common(src, "kspace_derivs_c64", written)
    assert loads == [("v", "fk")]
    params = _params(src, "kspace_derivs_c64")
    assert params[0] == "const float2* __restrict__ fk"
    tables = [p.split()[-1] for p in params if p.startswith("const double*")]
    want = [f"k1{ax}" for ax in "xyz" if f"pd{ax}" in mask]
    want += ["k2x", "k2y", "k2z"] if "lap" in mask else []
    assert tables == want
    assert params[-1] == "const double inv_n"
    # the double expressions are the complex128 form's
    c128 = hip.kspace_source("derivs", KSHAPE, outs=mask)
    for (p64, rhs64), (p128, rhs128) in zip(_stores(src), _stores(c128)):
        re_, im_ = re.fullmatch(r"make_double2\((.+), (.+)\)",
                                rhs128).groups()
        assert p64 == p128
        assert rhs64 == f"make_float2((float)({re_}), (float)({im_}))"
    assert src.count("rounded(") == c128.count("rounded(")
    if "lap" in mask:
        assert ("-((rounded(kx * kx) + rounded(ky * ky))\n"
                "                         + rounded(kz * kz));") in src


@pytest.mark.parametrize("mu", [0, 1, 2])
@pytest.mark.parametrize("accumulate", [False, True])
def test_div_accum_c64_source(mu, accumulate):
    src = hip.kspace_source("div_accum", KSHAPE, ctype="complex64", mu=mu,
                            accumulate=accumulate)
    loads = _check_common(src, "kspace_div_accum_c64", ["div_k"])
    assert loads == [("v", "fk")] + ([("d", "div_k")] if accumulate else [])
    assert _params(src, "kspace_div_accum_c64") == [
        "const float2* __restrict__ fk", "float2* __restrict__ div_k",
        "const double* __restrict__ k1", "const double inv_n"]
    assert f"k1[{('ii', 'jj', 'kk')[mu]}]" in src
    assert ("double2 term = make_double2((-q * v.y) * inv_n, "
            "(q * v.x) * inv_n);") in src
    assert ("d.x + rounded(term.x), d.y + rounded(term.y)" in src) \
        == accumulate
    assert _stores(src) == [
        ("div_k", "make_float2((float)(term.x), (float)(term.y))")]
    c128 = hip.kspace_source("div_accum", KSHAPE, mu=mu,
                             accumulate=accumulate)
    assert src.count("rounded(") == c128.count("rounded(")


def test_poisson_c64_source():
    src = hip.kspace_source("poisson", KSHAPE, ctype="complex64")
    loads = _check_common(src, "kspace_poisson_c64", ["sol"])
    assert loads == [("v", "rhok")]
    params = _params(src, "kspace_poisson_c64")
    # sol may be rhok: neither is declared restrict
    assert params[:2] == ["const float2* rhok", "float2* sol"]
    assert params[-2:] == ["const double inv_n", "const double m_squared"]
    c128 = hip.kspace_source("poisson", KSHAPE)
    shared = ["const double mk2 = (ex[ii] + ey[jj]) + ez[kk];",
              "const double den = mk2 - m_squared;",
              "    ? make_double2((v.x * inv_n) / den, (v.y * inv_n) / den)",
              "    : make_double2(0.0, 0.0);"]
    for line in shared:
        assert line in src and line in c128, line
    assert "const double2 r = (mk2 < 0.0)\n" in src
    assert _stores(src) == [("sol", "make_float2((float)(r.x), (float)(r.y))")]
    assert src.count("rounded(") == c128.count("rounded(")


@pytest.mark.parametrize("ident,op,flags", FORMS, ids=IDS)
def test_complex128_source_has_not_moved(ident, op, flags):
    src = hip.kspace_source(op, KSHAPE, **flags)
    assert src == hip.kspace_source(op, KSHAPE, ctype="complex128", **flags)
    assert src == hip.kspace_source(op, KSHAPE, torch.complex128, **flags)
    assert not re.search(r"\bfloat", src)
    assert f"void kspace_{op}(" in src
    assert hashlib.sha256(src.encode()).hexdigest() == SHA256_C128[ident]
    c64 = hip.kspace_source(op, KSHAPE, ctype="complex64", **flags)
    assert c64 != src and f"void kspace_{op}_c64(" in c64


def test_every_form_has_a_recorded_hash():
    assert len(FORMS) == 15 + 6 + 1 == len(SHA256_C128)
    assert set(IDS) == set(SHA256_C128)
    assert len(set(SHA256_C128.values())) == len(FORMS)


def test_unknown_storage_types_are_refused():
    for bad in ("float32", torch.float64, None, "complex32"):
        with pytest.raises(ValueError, match="ctype"):
            hip.kspace_source("poisson", KSHAPE, ctype=bad)
        with pytest.raises(ValueError, match="ctype"):
            hip.kspace_source("derivs", KSHAPE, bad, outs=("lap",))


def test_source_generation_needs_no_native_module(monkeypatch):
    def no_ext():
        raise AssertionError("kspace_source touched the native module")
    monkeypatch.setattr(hip, "ext", no_ext)
    for _, op, flags in FORMS:
        assert hip.kspace_source(op, KSHAPE, ctype="complex64", **flags)


HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
    else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_c64_sources_compile_for_gfx950(tmp_path):
    """Device-only cross-compilation of every complex64 source, to
    assembly: no scratch, every mode an 8-byte access, one store per
    output, and every load of a thread issued before its first store
    (the Poisson solve runs in place)."""
    procs = []
    for ident, op, flags in FORMS:
        form = ident.replace(":", "_").replace("+", "_")
        path = tmp_path / f"{form}.hip"
        path.write_text(hip.kspace_source(op, KSHAPE, ctype="complex64",
                                          **flags))
        procs.append((ident, form, op, flags, subprocess.Popen(
            [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3",
             "-include", "hip/hip_runtime.h",
             "-S", str(path), "-o", str(tmp_path / f"{form}.s")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for ident, form, op, flags, proc in procs:
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode == 0, (ident, out[-3000:])
        asm = (tmp_path / f"{form}.s").read_text()
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", asm), ident
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", asm).group(1))
        print(f"{ident}: {vgprs} VGPRs")
        # eight waves per SIMD need at most 64
        assert vgprs <= 64, (ident, vgprs)
        code = asm[:asm.index("s_endpgm")]
        ops = re.findall(r"^\s*(global_(?:load|store)_\w+)", code, re.M)
        loads = [i for i, o in enumerate(ops) if "load" in o]
        stores = [i for i, o in enumerate(ops) if "store" in o]
        assert loads and stores and max(loads) < min(stores), (ident, ops)
        nstore = len(flags["outs"]) if op == "derivs" else 1
        assert len(stores) == nstore, (ident, ops)
        assert all(ops[i] == "global_store_dwordx2" for i in stores), \
            (ident, ops)
        nmode = 2 if flags.get("accumulate") else 1
        assert [ops[i] for i in loads].count("global_load_dwordx2") \
            >= nmode, (ident, ops)

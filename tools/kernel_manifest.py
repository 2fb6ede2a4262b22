#!/usr/bin/env python
"""What backend/hip.py generates and launches, as text that can be diffed.

Without arguments: the HIP source of every kernel family at the small
fixed inputs of the source tests, as sorted JSON ``{identifier:
sha256(source)}``.  Needs no device and no native module: kernels that
have no ``*_source`` function are built against a stand-in for
``hip.ext`` that records what would compile.  ``tests/kernel_manifest.json``
is this output; a change that means to move a kernel regenerates it
(``python tools/kernel_manifest.py -o tests/kernel_manifest.json``) and
the diff names the kernels it touched.

With ``--launches``, on a GPU: one launch per family through the real
native module, wrapped in a recorder.  One line per launch: the kernel's
name and source hash, grid, block, dynamic LDS, the pointers (each as the
position of the argument tensor it equals, not as an address), the ints
and the doubles.  Run it before and after a change to the host plumbing
and diff the two outputs.
"""

import argparse
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from pystella_amd.backend import hip                            # noqa: E402
from pystella_amd.field import (                                # noqa: E402
    Field, get_field_args, shift_fields, var)
from pystella_amd.field import expr as ex                       # noqa: E402

RANK_SHAPE, HALO = (12, 10, 8), 2
DTYPES = {"float64": torch.float64, "float32": torch.float32}
CTYPES = ("complex128", "complex64")


def _sha(src):
    return hashlib.sha256(src.encode()).hexdigest()


class _SourceOnly:
    """Stands in for the native module: records what would compile."""

    def __init__(self):
        self.sources = {}

    def jit_compile(self, src, name):
        self.sources[name] = src
        return name


# -- the maps of the source tests --------------------------------------------

def _elementwise_map():
    """tests/test_kspace_map_source.py ``_existing_sources``."""
    f, g = Field("f", offset="h", shape=(2,)), Field("g")
    a = var("a")
    stmts = {g: a * f[0]**2 + ex.exp(-f[1]) / (1 + ex.fabs(f[0]))}
    entries = [(a * f[0] * f[1], "sum"), (f[1]**3, "max")]
    return stmts, entries, f


def _stencil_map(h=HALO):
    """tests/test_jit_maps_edges.py ``test_stencil_partial_tiles``."""
    r1, r2 = (h + 1) // 2, h
    f, g = Field("f", offset="h"), Field("g", offset="h")
    out = Field("out", offset=0)
    return {out: (
        2.0 * f
        + shift_fields(f, (r1, 0, 0)) + shift_fields(f, (-r2, 0, 0))
        + 0.5 * (shift_fields(f, (0, r1, 0)) + shift_fields(f, (0, -r2, 0)))
        + 0.25 * (shift_fields(f, (0, 0, r2)) + shift_fields(f, (0, 0, -r1)))
        + 0.125 * shift_fields(f, (r1, r1, 0))
        + shift_fields(g, (0, r2, -r1)) * var("c"))}


def _generic_kernels(dtype):
    """{family: kernel} of the generic JIT maps for ``dtype``."""
    stmts, entries, f = _elementwise_map()
    args = get_field_args(stmts)
    halo = (HALO,) * 3
    out = {
        "elementwise": hip.JitElementwise(
            stmts, {}, args, ["a"], halo, RANK_SHAPE, dtype=dtype),
        "reduction": hip.JitReduction(
            entries, get_field_args([f]), ["a"], halo, RANK_SHAPE,
            dtype=dtype),
    }
    smap = _stencil_map()
    out["stencil"] = hip.JitStencil(
        smap, {}, get_field_args(smap), ["c"], halo, RANK_SHAPE, dtype=dtype)
    if dtype == torch.float64:
        out["stage_reduction"] = hip.JitStageReduction(
            stmts, {}, entries, args, ["a"], halo, RANK_SHAPE)
    return out


def _friedmann():
    return hip.JitFriedmann(5, 60, [1., 1., 1., 1., 1.],
                            [1., 1., -1 / 3, -1 / 3, -1.],
                            float(np.prod(RANK_SHAPE)))


def _wrap_source(rank_shape, h, nf, axes, dtype):
    if hasattr(hip, "wrap_source"):
        return hip.wrap_source(rank_shape, h, nf, axes, dtype)
    # before wrap_source existed: the text as wrap_star formatted it
    defines = hip.geometry_defines(h, rank_shape, rtype=hip._RTYPE[dtype])
    defines += f"#define NF {nf}\n"
    for ax, nm in enumerate("XYZ"):
        defines += f"#define WRAP{nm} {1 if ax in axes else 0}\n"
    name = f"wrap_star_{h}_{nf}_" + "".join(
        str(int(ax in axes)) for ax in range(3))
    return name, hip.WRAP_TEMPLATE.format(defines=defines, name=name)


def _stage_sources(h, dtype):
    """The forms of tests/test_stage_fp32_source.py ``sources``, and the
    device-loop kernel without nontemporal accesses."""
    from tests import test_stage_fp32_source as t
    out = {form: src for form, (src, _) in t.sources(h, dtype).items()}
    st, _ = t.components(h)
    kern, = st._stepper.steps[1].ring_kernels(
        t.GRID, DTYPES[dtype], state_map=t.STATE_MAP, nt=False,
        compile=False)
    out["plain_nt0"] = kern.source
    return out


def build_manifest():
    """{identifier: sha256 of the generated source}."""
    from tests import test_histogram_source as t_hist
    from tests import test_kspace_c64_source as t_ksp
    from tests import test_mg_transfer_source as t_mg
    from tests import test_obs_c64_source as t_obs
    from tests import test_rayleigh_source as t_ray
    from tests.kspace_map_reference import CASES, KSHAPE

    real_ext, fake = hip.ext, _SourceOnly()
    hip.ext = lambda: fake
    src = {}
    try:
        for dname, dtype in DTYPES.items():
            for fam, k in _generic_kernels(dtype).items():
                src[f"{fam}:{dname}"] = k.source
            for template in t_hist.TEMPLATES:
                src[f"histogram:{template}:{dname}"] = \
                    t_hist._kernel(template, dname).source
            for h in (1, 2):
                for form, s in _stage_sources(h, dname).items():
                    src[f"lap_stage:h{h}:{dname}:{form}"] = s
        src["friedmann"] = _friedmann().source
        for name, case in CASES.items():
            for form in ("double", "mixed"):
                dtypes = {n: np.dtype(d).name
                          for n, d in case.forms[form].items()}
                src[f"kspace_map:{name}:{form}"] = hip.JitKspaceMap(
                    case.statements, case.tmp,
                    get_field_args({**case.tmp, **case.statements}), dtypes,
                    KSHAPE, name=case.name, compile=False).source
    finally:
        hip.ext = real_ext
    for r in range(4):
        for axes in itertools.combinations(range(3), r):
            for dname, dtype in DTYPES.items():
                src[f"wrap:{''.join('xyz'[a] for a in axes) or 'none'}:"
                    f"{dname}"] = _wrap_source(RANK_SHAPE, HALO, 2, axes,
                                               dtype)[1]
    for ct in CTYPES:
        src[f"spectra_bin:{ct}"] = hip.spectra_bin_source(700, ctype=ct)
        for op, tak in t_obs.VARIANTS:
            src[f"projector:{op}:{int(tak)}:{ct}"] = hip.projector_source(
                op, t_obs.KSHAPE, tak, ctype=ct)
        for ident, op, flags in t_ksp.FORMS:
            src[f"kspace:{ident}:{ct}"] = hip.kspace_source(
                op, t_ksp.KSHAPE, ctype=ct, **flags)
        for wkb, is_real in itertools.product((False, True), repeat=2):
            for random in (True, False):
                src[f"rayleigh:{int(wkb)}{int(is_real)}{int(random)}:{ct}"] \
                    = t_ray._source(wkb, is_real, ct, random=random)
    for form, dname, correct in t_mg.FORMS:
        src[f"mg:{form}:{dname}:{int(correct)}"] = t_mg._source(
            form, dname, correct)
    return {ident: _sha(s) for ident, s in sorted(src.items())}


# -- launches -----------------------------------------------------------------

class _Recorder:
    """The native module with ``jit_compile`` and ``jit_launch`` noted."""

    def __init__(self, native):
        self.native = native
        self.names = {}
        self.lines = []
        self.case = None
        self.tensors = []

    def __getattr__(self, name):
        return getattr(self.native, name)

    def jit_compile(self, src, name):
        key = self.native.jit_compile(src, name)
        self.names[key] = f"{name} {_sha(src)[:16]}"
        return key

    def jit_launch(self, key, gx, gy, gz, bx, by, bz, shmem, stream, ptrs,
                   ints, doubles):
        where = {t.data_ptr(): i for i, t in enumerate(self.tensors)}
        self.lines.append(
            f"{self.case}: {self.names[key]} grid=({gx},{gy},{gz}) "
            f"block=({bx},{by},{bz}) shmem={shmem} ptrs="
            f"{[where.get(p, 'own') for p in ptrs]} ints={list(ints)} "
            f"doubles={[repr(float(d)) for d in doubles]}")
        self.native.jit_launch(key, gx, gy, gz, bx, by, bz, shmem, stream,
                               ptrs, ints, doubles)


def record_launches():
    """One case per family at the smallest shapes of the GPU tests."""
    from tests import test_stage_fp32_source as t_stage
    from tests.kspace_map_reference import CASES, KSHAPE
    from pystella_amd.multigrid.transfer import (
        FullWeighting, LinearInterpolation)

    rec = _Recorder(hip.ext())
    real_ext = hip.ext
    hip.ext = lambda: rec
    gen = torch.Generator().manual_seed(11)

    def rand(shape, dtype=torch.float64):
        real = torch.rand(tuple(shape), dtype=torch.float64, generator=gen)
        if dtype.is_complex:
            real = torch.complex(real, real.flip(-1))
        return (real + 0.5).to(dtype).cuda().contiguous()

    def case(name, *tensors):
        rec.case, rec.tensors = name, list(tensors)

    try:
        pad = tuple(n + 2 * HALO for n in RANK_SHAPE)
        f, g = rand((2,) + pad), rand(RANK_SHAPE)
        kernels = _generic_kernels(torch.float64)
        for fam in ("elementwise", "reduction", "stage_reduction"):
            case(fam, f, g)
            kernels[fam]({"f": f, "g": g, "a": 1.5})
        f1, g1, out = rand(pad), rand(pad), rand(RANK_SHAPE)
        case("stencil", f1, g1, out)
        kernels["stencil"]({"f": f1, "g": g1, "out": out, "c": 1.5})

        from tests import test_histogram_source as t_hist
        hpad = tuple(n + 2 * t_hist.H for n in t_hist.RANK_SHAPE)
        hf, hg = rand(hpad) - 0.5, rand(t_hist.RANK_SHAPE) - 0.5
        for template, num_bins in t_hist.TEMPLATES.items():
            pairs = t_hist._pairs(num_bins)
            k = hip.JitHistogram(
                pairs, num_bins,
                get_field_args([e for pair in pairs for e in pair]), ["c"],
                (t_hist.H,) * 3, t_hist.RANK_SHAPE)
            case(f"histogram:{template}", hf, hg)
            k({"f": hf, "g": hg, "c": 2.0})

        st, red = t_stage.components(2)
        grid = t_stage.GRID
        env = {n: (t.cuda() if isinstance(t, torch.Tensor) else t)
               for n, t in t_stage._env(
                   2, dict.fromkeys(("f", "f_next", "dfdt", "f_tmp",
                                     "dfdt_tmp"), torch.float64)).items()}
        env["f"] += 0.2
        env["state"][0] = 1.0
        names = ("f", "f_next", "dfdt", "f_tmp", "dfdt_tmp", "state")
        kern, = st._stepper.steps[1].ring_kernels(
            grid, torch.float64, state_map=t_stage.STATE_MAP)
        slabs = t_stage._slabs(2)
        nblk = kern.shell_nblk(slabs)
        partials = torch.zeros((len(kern.entries), nblk + kern.nblk),
                               dtype=torch.float64, device="cuda")
        case("lap_stage:call", *(env[n] for n in names))
        kern(env)
        case("lap_stage:box", *(env[n] for n in names), partials)
        kern.launch_box(env, (2, 70, 2, 9, 2, 78), partials, nblk,
                        nblk + kern.nblk)
        case("lap_stage:shell", *(env[n] for n in names), partials)
        kern.launch_shell(env, slabs, partials, 0, nblk + kern.nblk)
        host, = st._stepper.steps[0].ring_kernels(grid, torch.float64)
        case("lap_stage:host", *(env[n] for n in names))
        host(dict(env, a=1.0, hubble=0.1))
        lap = torch.zeros((2,) + grid, dtype=torch.float64, device="cuda")
        k = red[True].lap_reduction_kernel(grid, 2)
        case("lap_reduction", env["f"], env["dfdt"], lap)
        k({"f": env["f"], "dfdt": env["dfdt"], "lap_f": lap, "a": 1.0})

        fk_ = _friedmann()
        sums = torch.zeros(5, dtype=torch.float64, device="cuda")
        part = rand((5, 60))
        state = rand((8,))
        case("friedmann", part, sums, state)
        fk_.finish_sums(part, sums)
        fk_.step(sums, state, 0.5, 0.25, 1e-3)

        case("wrap", f)
        hip.wrap_star(f, HALO, (0, 1, 2))

        n = int(np.prod(KSHAPE))
        wbase = rand((n,))
        bidx = (torch.arange(n, dtype=torch.int32) % 37).cuda()
        eff = [rand((m,)) for m in KSHAPE]
        for ct in CTYPES:
            cdtype = getattr(torch, ct)
            c64 = "_c64" if ct == "complex64" else ""
            fk, vec = rand(KSHAPE, cdtype), rand((3,) + KSHAPE, cdtype)
            outs = {o: rand(KSHAPE, cdtype) for o in ("pdx", "lap")}
            plus, minus = rand(KSHAPE, cdtype), rand(KSHAPE, cdtype)
            case(f"spectra_bin:{ct}", fk.reshape(-1), wbase, bidx)
            getattr(hip, "spectra_bin" + c64)(fk.reshape(-1), wbase, bidx, 37)
            case(f"projector:{ct}", vec, plus, minus, *eff)
            if c64:
                hip.projector_op_c64("vec_to_pol", KSHAPE,
                                     [vec, plus, minus], eff)
            else:
                hip.projector_op("vec_to_pol", KSHAPE,
                                 [t.data_ptr() for t in (vec, plus, minus)],
                                 eff)
            case(f"kspace:{ct}", fk, plus, outs["pdx"], outs["lap"], *eff)
            getattr(hip, "kspace_derivs" + c64)(fk, outs, eff, eff, 1 / n)
            getattr(hip, "kspace_div_accum" + c64)(
                fk, plus, eff[1], 1, 1 / n, True)
            getattr(hip, "kspace_poisson" + c64)(fk, fk, *eff, 1 / n, 0.25)
            sp, om = rand(KSHAPE), rand(KSHAPE)
            tabs = [torch.arange(m, dtype=torch.int32).cuda()
                    for m in KSHAPE]
            case(f"rayleigh:{ct}", fk, plus, sp, om, *tabs)
            hip.rayleigh_modes(fk, None, sp, None, tabs, (12, 10, 14),
                               0x1234567890abcdef, 3, is_real=True)
            hip.rayleigh_modes(fk, plus, sp, om, tabs, (12, 10, 14),
                               0xfedcba0987654321, 4, 0.3, is_real=True,
                               random=False)

        kcase = CASES["filter"]
        dtypes = {n: np.dtype(d).name
                  for n, d in kcase.forms["mixed"].items()}
        inputs = {n: torch.from_numpy(a).cuda()
                  for n, a in kcase.inputs(KSHAPE, "mixed").items()}
        k = hip.JitKspaceMap(
            kcase.statements, kcase.tmp,
            get_field_args({**kcase.tmp, **kcase.statements}), dtypes, KSHAPE,
            name=kcase.name)
        case("kspace_map", *(inputs[n] for n in sorted(inputs)))
        k({**inputs, **kcase.scalars})

        for dtype in DTYPES.values():
            mf1, mf2 = rand((2, 12, 10, 14), dtype), rand((2, 7, 6, 8), dtype)
            case(f"mg:{dtype}", mf1, mf2)
            fw, li = FullWeighting(1), LinearInterpolation(1)
            hip.mg_restrict(mf1, mf2, fw.coefs, 1, False)
            hip.mg_interpolate(mf1, mf2, li.even, li.odd, 1, True)
        torch.cuda.synchronize()
    finally:
        hip.ext = real_ext
    return rec.lines


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--launches", action="store_true",
                   help="record one launch per family (needs a GPU)")
    p.add_argument("-o", "--output", help="write here instead of stdout")
    args = p.parse_args()
    if args.launches:
        text = "\n".join(record_launches()) + "\n"
    else:
        text = json.dumps(build_manifest(), indent=1, sort_keys=True) + "\n"
    if args.output:
        with open(args.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()

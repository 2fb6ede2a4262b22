"""GPU execution: AOT CDNA4 kernels + hiprtc-JIT'd kernel templates.

This module is the only place that touches the native extension
(``pystella_amd._C``).  Policy: on a GPU box the HIP path is the one
that runs — if the extension is missing or fails to load, GPU calls
raise immediately (no silent torch fallback; see repo instructions on
native-code loading).

Layout, top to bottom:

* the host plumbing, written once: ``_JitKernel`` (parameter list,
  compile or source only, argument checks, launch) with
  ``_PartialsKernel`` for the kernels that leave per-block partials, and
  for the function-style families ``_cached_kernel``, ``_launch_1d``,
  ``_check_arg`` and ``_kshape_defines``;
* the JIT families, each a template, its source generator (a ``Jit*``
  class or a ``*_source`` function, none of which needs a device) and
  its launch: elementwise, stencil, stage-reduction, wrap, reduction,
  histogram, spectra binning, projectors, k-space derivatives and
  Poisson, k-space maps, Rayleigh modes, multigrid transfers, the
  register-ring Laplacian kernels and the Friedmann update;
* the wrappers of the AOT kernels in csrc/ (``derivs``, ``divergence``,
  ``tt_project_c64``).

``tools/kernel_manifest.py`` hashes every family's generated source and
records every family's launch arguments; a change here that means to
move no kernel leaves both outputs as they were.
"""

from __future__ import annotations

import math
import os

import numpy as np
import torch

from pystella_amd.backend.codegen import (
    Codegen, KspaceCodegen, KSPACE_DTYPES, KSPACE_PREAMBLE, PREAMBLE,
    geometry_defines,
)

_EXT = None


def ext():
    global _EXT
    if _EXT is None:
        from pystella_amd.backend import build as _build
        if _build.needs_rebuild():
            # sources newer than the shipped .so (e.g. edited after the
            # last build) — rebuild in place rather than run stale code
            _build.build_extension()
        try:
            from pystella_amd import _C
        except ImportError as e:
            raise ImportError(
                "pystella_amd._C native extension not built; run "
                "`python -m pystella_amd.backend.build` (hipcc, gfx950). "
                f"Underlying error: {e}") from e
        _C.set_cache_dir(_jit_cache_dir())
        _EXT = _C
    return _EXT


def _jit_cache_dir():
    """Directory of the on-disk hiprtc code cache: PYSTELLA_JIT_CACHE
    if set; else the first of the package tree, the user's cache
    directory and a per-user directory under the system temp dir that
    this user can write (the package may be installed or checked out
    read-only, or belong to another user).  "" (no disk cache, kernels
    are compiled once per process) if none is writable."""
    import tempfile
    cache = os.environ.get("PYSTELLA_JIT_CACHE")
    if cache:
        os.makedirs(cache, exist_ok=True)
        return cache
    uid = os.getuid()
    candidates = [
        os.path.join(os.path.dirname(os.path.dirname(
            os.path.abspath(__file__))), ".hiprtc_cache"),
        os.path.join(
            os.environ.get("XDG_CACHE_HOME")
            or os.path.join(os.path.expanduser("~"), ".cache"),
            "pystella_amd", "hiprtc"),
        os.path.join(tempfile.gettempdir(),
                     f"pystella_amd-hiprtc-{uid}"),
    ]
    for cand in candidates:
        try:
            os.makedirs(cand, mode=0o700, exist_ok=True)
        except OSError:
            continue
        if not os.access(cand, os.W_OK | os.X_OK):
            continue
        # a predictable name in a shared temp dir: only if it is ours
        if cand is candidates[-1] and os.stat(cand).st_uid != uid:
            continue
        return cand
    return ""


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_tensor(name, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"argument {name} must be a CUDA tensor, got "
                        f"{type(t)}")
    if not t.is_contiguous():
        raise ValueError(f"argument {name} must be contiguous")
    return t


def _resolve_scalar(env, key):
    if isinstance(key, tuple):
        name, idx = key
        v = env[name]
        if isinstance(v, torch.Tensor):
            return float(v.reshape(-1)[np.ravel_multi_index(
                idx, v.shape)] if v.numel() > 1 else v.item())
        v = np.asarray(v)
        if v.ndim == 0 or v.size == 1:
            return float(v.reshape(-1)[0])
        return float(v[idx])
    v = env[key]
    if isinstance(v, torch.Tensor):
        return float(v.item())
    return float(np.asarray(v).reshape(-1)[0])


# ---------------------------------------------------------------------------
# host plumbing of the JIT kernels, written once

_RTYPE = {torch.float64: "double", torch.float32: "float"}


def _spatial(field_args):
    return [fa for fa in field_args if fa.spatial]


class _JitKernel:
    """Host side of a generated kernel: its C parameter list, compiling
    it (or only keeping its source), checking its arguments and
    launching it.

    csrc/module.cpp's ``jit_launch`` passes the pointers, then the ints,
    then the doubles.  :meth:`_declare` writes the signature in that
    order and records the pointers' names and the scalars' keys in the
    order it wrote them; :meth:`_pointers` and :meth:`_launch` read only
    what it recorded.  So the order is decided here and nowhere else,
    and a signature cannot disagree with its launch.  What the
    environment does not name (the ``partials`` or ``hist`` buffer a
    kernel allocates itself, a block of ints) is ``extra`` text to
    ``_declare`` and follows the gathered pointers, or goes as ``ints``,
    in the ``_launch`` call of the class that declared it.
    """

    # dynamic LDS of every launch
    shmem = 0
    # ``want``/``short`` are the expected dtype with and without "torch."
    _dtype_error = ("argument {name} has dtype {got}, kernel compiled for "
                    "{want}")

    def _declare(self, cg, names, ptr, extra=(), scalar="double", sep=", "):
        """The parameter list: pointers ``names`` declared ``ptr``
        (``ptr __restrict__ name``, or what ``ptr(name)`` returns), the
        ``extra`` declarations, then the run-time scalars that ``cg`` has
        collected (so call this after the last emission)."""
        self.ptr_names = list(names)
        self.scalar_keys = [k for _, k in cg.scalars]
        if not callable(ptr):
            ptr = (ptr + " __restrict__ {}").format
        return sep.join([ptr(n) for n in names] + list(extra)
                        + [f"{scalar} {c}" for c, _ in cg.scalars])

    def _declare_fields(self, cg, field_args, ptr, extra=()):
        """:meth:`_declare` for the spatial ``field_args``, in their
        order."""
        self.field_args = _spatial(field_args)
        return self._declare(cg, [fa.name for fa in self.field_args], ptr,
                             extra)

    def _build(self, src, name, compile):
        """``compile=False``: source only, inspectable without a device;
        such a kernel cannot be launched."""
        self.source = src
        self.key = ext().jit_compile(src, name) if compile else None

    def _tiled(self, tile, rank_shape):
        """Launch shape of a (TBZ, TBY, XCHUNK) tiling of the grid."""
        self.grid = _tile_grid(tile, rank_shape)
        self.block = tile[0] * tile[1]

    def _require_compiled(self):
        if self.key is None:
            raise RuntimeError(
                f"{type(self).__name__} was built with compile=False "
                "(source only) and cannot be launched")

    def _arg_dtype(self, name):
        """The dtype the kernel reads pointer ``name`` as."""
        return self.dtype

    def _pointers(self, env):
        """(pointers, device) of the kernel's array arguments.  Every
        dtype is looked at first, before the device: the kernel would
        read a buffer of another dtype as its own type, garbage, and
        past the end of a narrower one."""
        self._require_compiled()
        for n in self.ptr_names:
            t, want = env[n], self._arg_dtype(n)
            if isinstance(t, torch.Tensor) and t.dtype != want:
                raise TypeError(self._dtype_error.format(
                    name=n, got=t.dtype, want=want, short=str(want)[6:]))
        ptrs, dev = [], None
        for n in self.ptr_names:
            t = _check_tensor(n, env[n])
            dev = t.device
            ptrs.append(t.data_ptr())
        return ptrs, dev

    def _launch(self, key, grid, env, ptrs, ints=()):
        doubles = [_resolve_scalar(env, k) for k in self.scalar_keys]
        ext().jit_launch(key, grid[0], grid[1], grid[2], self.block, 1, 1,
                         self.shmem, _stream(), ptrs, list(ints), doubles)

    def __call__(self, env):
        ptrs, _ = self._pointers(env)
        self._launch(self.key, self.grid, env, ptrs)


class _PartialsKernel(_JitKernel):
    """A kernel whose blocks each leave one column of a float64
    ``[nred, nblk]`` partials buffer (PARTIALS_TAIL), finished with
    torch ops and one packed copy to the host."""

    PARTIALS = "double* __restrict__ partials"

    def _tiled(self, tile, rank_shape):
        super()._tiled(tile, rank_shape)
        self.nblk = self.grid[0] * self.grid[1] * self.grid[2]
        self._partials = None

    def launch_only(self, env, ints=()):
        """Full-grid launch without finishing the reduction; returns the
        raw per-block partials tensor [nred, nblk] that the kernel owns
        (stream-ordered, no host synchronization).  It is allocated anew
        when the device or the block count changed."""
        ptrs, dev = self._pointers(env)
        p = self._partials
        if p is None or p.device != dev or p.shape[1] != self.nblk:
            p = self._partials = torch.empty(
                (len(self.entries), self.nblk), dtype=torch.float64,
                device=dev)
        self._launch(self.key, self.grid, env, ptrs + [p.data_ptr()], ints)
        return p

    def _finish(self, dev):
        """Combine per-block partials on-device, one packed D2H copy."""
        vals = torch.empty(len(self.entries), dtype=torch.float64,
                           device=dev)
        for r, (_, op) in enumerate(self.entries):
            row = self._partials[r]
            if op in ("sum", "avg"):
                vals[r] = row.sum()
            elif op == "prod":
                vals[r] = row.prod()
            elif op == "max":
                vals[r] = row.max()
            else:
                vals[r] = row.min()
        return vals.cpu().tolist()

    def __call__(self, env):
        return self._finish(self.launch_only(env).device)


# the generic reductions word their dtype refusal in their own way
_REDUCTION_DTYPE_ERROR = ("reduction argument '{name}' has dtype {got}, "
                          "kernel expects {want}")


# what the function-style families share

def _cached_kernel(cache, key, name, make_source):
    """The compiled kernel ``name`` under ``cache[key]``, compiled from
    ``make_source()`` on first use."""
    kid = cache.get(key)
    if kid is None:
        kid = cache[key] = ext().jit_compile(make_source(), name)
    return kid


def _blocks_1d(n, cap=None):
    blocks = (n + 255) // 256
    return blocks if cap is None else min(cap, blocks)


def _launch_1d(kid, n, ptrs, ints=(), doubles=(), cap=None):
    """Blocks of 256 threads over ``n`` sites, at most ``cap`` blocks."""
    ext().jit_launch(kid, _blocks_1d(n, cap), 1, 1, 256, 1, 1, 0, _stream(),
                     ptrs, list(ints), list(doubles))


def _kshape_defines(kshape):
    return (f"#define NKX {kshape[0]}\n"
            f"#define NKY {kshape[1]}\n"
            f"#define NKZ {kshape[2]}\n"
            "#define VOLK ((long)NKX * NKY * NKZ)\n")


def _check_arg(name, t, dtype, why, shape=None, ndim=None, numel=None):
    """A contiguous device tensor of ``dtype`` (one, or a tuple of the
    allowed ones), else a TypeError ending in ``why``; optionally of
    ``shape``, of ``ndim`` dimensions, or of ``numel = (count, wording)``
    elements."""
    _check_tensor(name, t)
    if t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise TypeError(f"argument {name} has dtype {t.dtype}{why}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"argument {name} has shape {tuple(t.shape)}, "
                         f"expected {tuple(shape)}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"argument {name} has shape {tuple(t.shape)}, "
                         f"expected a {ndim}-D k-space array")
    if numel is not None and t.numel() != numel[0]:
        raise ValueError(f"argument {name} has {t.numel()} elements, "
                         f"{numel[1]} {numel[0]}")
    return t


# ---------------------------------------------------------------------------
# JIT'd elementwise map (fused RK stage kernels etc.)

ELEMENTWISE_TEMPLATE = """{defines}
{preamble}
extern "C" __global__ __launch_bounds__(TBZ * TBY) void {name}(
    {params})
{{
    const int k = blockIdx.x * TBZ + (threadIdx.x % TBZ);
    const int j = blockIdx.y * TBY + (threadIdx.x / TBZ);
    if (k >= NZ || j >= NY) return;
    const int i0 = blockIdx.z * XCHUNK;
    const int i1 = (i0 + XCHUNK < NX) ? i0 + XCHUNK : NX;
    for (int i = i0; i < i1; ++i) {{
        {body}
    }}
}}
"""


def _tile_defines(tile):
    tbz, tby, xchunk = tile
    return (f"#define TBZ {tbz}\n#define TBY {tby}\n"
            f"#define XCHUNK {xchunk}\n")


def _tile_grid(tile, rank_shape):
    tbz, tby, xchunk = tile
    nx, ny, nz = rank_shape
    return ((nz + tbz - 1) // tbz, (ny + tby - 1) // tby,
            (nx + xchunk - 1) // xchunk)


class JitElementwise(_JitKernel):
    """Compiled fused per-site map over the interior grid.  Supports
    fp64 and fp32 arrays (``using real = double|float`` baked into the
    kernel; run-time scalars stay double and are cast on use)."""

    def __init__(self, map_dict, tmp_instructions, field_args, scalar_names,
                 halo, rank_shape, name="ew_map", tile=(64, 4, 64),
                 dtype=torch.float64, compile=True):
        self.rank_shape = tuple(rank_shape)
        self.tile = tile
        self.dtype = dtype
        cg = Codegen(field_args, halo, rank_shape)
        body = cg.emit_statements(map_dict, tmp_instructions)
        params = self._declare_fields(cg, field_args, "real*")
        self._build(ELEMENTWISE_TEMPLATE.format(
            defines=geometry_defines(halo, rank_shape,
                                     rtype=_RTYPE[dtype])
            + _tile_defines(tile),
            preamble=PREAMBLE, name=name, params=params, body=body),
            name, compile)
        self._tiled(tile, rank_shape)


def get_elementwise_kernel(map_dict, tmp_instructions, field_args,
                           scalar_names, halo, rank_shape, name="ew_map",
                           tile=(64, 4, 64), dtype=torch.float64):
    return JitElementwise(map_dict, tmp_instructions, field_args,
                          scalar_names, halo, rank_shape, name=name,
                          tile=tile, dtype=dtype)


# ---------------------------------------------------------------------------
# Generic LDS-staged stencil kernel: x-marching blocks stage each
# neighbor-read field's current x-plane tile (with the ±H ghost rim)
# into LDS and serve pure-x shifts from a per-thread register ring —
# the generic-expression analogue of csrc/derivs.hip's
# gradlap_lds_knl (measured 17 % faster than plain L1 reuse for the
# isolated Laplacian, profiles/r01_lds_vs_ring.txt).  This is the
# CDNA4 realization of the reference's ``Stencil``/``StreamingStencil``
# workgroup-prefetch kernels (reference stencil.py:36-141).

STENCIL_TEMPLATE = """{defines}
{preamble}
extern "C" __global__ __launch_bounds__(SBZ * SBY) void {name}(
    {params})
{{
{lds_decls}
    const int lz = (int)(threadIdx.x % SBZ);
    const int ly = (int)(threadIdx.x / SBZ);
    const int k = blockIdx.x * SBZ + lz;
    const int j = blockIdx.y * SBY + ly;
    const int i0 = blockIdx.z * SXCHUNK;
    const int i1 = (i0 + SXCHUNK < NX) ? i0 + SXCHUNK : NX;
    const bool active = (k < NZ) && (j < NY);
    const int jc = j < NY ? j : NY - 1;
    const int kc = k < NZ ? k : NZ - 1;
    (void)jc; (void)kc;
{ring_init}
    for (int i = i0; i < i1; ++i) {{
{ring_load}
        __syncthreads();
        for (int t = (int)threadIdx.x; t < (SBY + 2*H) * (SBZ + 2*H);
             t += SBZ * SBY) {{
            const int tz = t % (SBZ + 2*H);
            const int ty = t / (SBZ + 2*H);
            int gj = blockIdx.y * SBY + ty;
            int gk = blockIdx.x * SBZ + tz;
            if (gj > NY + 2*H - 1) gj = NY + 2*H - 1;
            if (gk > NZ + 2*H - 1) gk = NZ + 2*H - 1;
            const long goff = (long)(i + H) * PSY * PSZ
                              + (long)gj * PSZ + gk;
{stage}
        }}
        __syncthreads();
        if (active) {{
            {body}
        }}
{ring_shift}
    }}
}}
"""


class _StencilCodegen(Codegen):
    """Codegen redirecting reads of prefetched components: (sy,sz)
    shifts -> LDS tile, pure-x shifts -> register ring."""

    def __init__(self, field_args, halo, rank_shape, tiles, rings):
        super().__init__(field_args, halo, rank_shape)
        self.tiles = tiles      # set of (name, lin)
        self.rings = rings      # set of (name, lin)
        self.store_ctx = False

    def field_access(self, f, outer_idx):
        if (not self.store_ctx and f.is_spatial and f.is_padded
                and len(outer_idx) <= 1):
            lin = int(outer_idx[0]) if outer_idx else 0
            sx, sy, sz = f.shift
            if sx == 0 and (f.name, lin) in self.tiles:
                return (f"t_{f.name}_{lin}[(ly + H + ({sy}))"
                        f" * (SBZ + 2*H) + (lz + H + ({sz}))]")
            if sy == 0 and sz == 0 and (f.name, lin) in self.rings:
                return f"r_{f.name}_{lin}[H + ({sx})]"
        return super().field_access(f, outer_idx)


class JitStencil(_JitKernel):
    """Compiled LDS-staged stencil map (see STENCIL_TEMPLATE)."""

    SBZ, SBY = 32, 8

    def __init__(self, map_dict, tmp_instructions, field_args,
                 scalar_names, halo, rank_shape, name="stencil_map",
                 xchunk=32, dtype=torch.float64, compile=True):
        from pystella_amd.field import (
            Field, Subscript, iter_exprs, walk_expr)
        self.rank_shape = tuple(rank_shape)
        self.dtype = dtype
        h = max(halo) if isinstance(halo, (tuple, list)) else halo

        # classify padded-field reads by shift pattern
        padded = {fa.name for fa in _spatial(field_args) if fa.padded}
        read_yz = set()      # (name, lin) with a (sy|sz)!=0 read
        read_x = set()       # (name, lin) with a pure-x != 0 read
        stores = set()       # components written (never prefetch)

        def scan(x, into_yz=read_yz, into_x=read_x):
            f = None
            lin = 0
            if isinstance(x, Subscript) and isinstance(x.aggregate, Field):
                f = x.aggregate
                if len(x.index) == 1 and isinstance(x.index[0], int):
                    lin = int(x.index[0])
                elif x.index:
                    return
            elif isinstance(x, Field):
                if x.shape:
                    # the aggregate of a subscript seen above, not a
                    # read of component 0
                    return
                f = x
            if f is None or f.name not in padded or not f.is_spatial:
                return
            sx, sy, sz = f.shift
            if sy or sz:
                into_yz.add((f.name, lin))
            elif sx:
                into_x.add((f.name, lin))

        exprs = list((tmp_instructions or {}).values()) \
            + list(map_dict.values())
        for e in iter_exprs(exprs):
            walk_expr(e, scan)
        for lhs in map_dict:
            f = lhs.aggregate if isinstance(lhs, Subscript) else lhs
            lin = (int(lhs.index[0]) if isinstance(lhs, Subscript)
                   and lhs.index and isinstance(lhs.index[0], int) else 0)
            if isinstance(f, Field):
                stores.add((f.name, lin))
        # a stored component cannot be served from stale LDS/ring
        tiles = read_yz - stores
        rings = read_x - stores

        sbz, sby = self.SBZ, self.SBY
        tile_doubles = (sby + 2 * h) * (sbz + 2 * h)
        esize = 8 if dtype == torch.float64 else 4
        self.lds_bytes = len(tiles) * tile_doubles * esize
        if self.lds_bytes > 48 * 1024:
            raise ValueError("stencil LDS tiles exceed budget")

        cg = _StencilCodegen(field_args, halo, rank_shape, tiles, rings)

        lds_decls, stage, ring_init, ring_load, ring_shift = \
            [], [], [], [], []
        for nm, lin in sorted(tiles):
            lds_decls.append(
                f"    __shared__ real t_{nm}_{lin}"
                f"[(SBY + 2*H) * (SBZ + 2*H)];")
            base = f"{nm} + {lin}L * PVOL" if lin else nm
            stage.append(
                f"            t_{nm}_{lin}[t] = ({base})[goff];")
        for nm, lin in sorted(rings):
            base = f"{nm} + {lin}L * PVOL" if lin else nm
            ring_init.append(
                f"    real r_{nm}_{lin}[2*H + 1];\n"
                f"    for (int p = 0; p < 2*H; ++p)\n"
                f"        r_{nm}_{lin}[p] = ({base})["
                f"(long)(i0 + p) * PSY * PSZ"
                f" + (long)(jc + H) * PSZ + (kc + H)];")
            ring_load.append(
                f"        r_{nm}_{lin}[2*H] = ({base})["
                f"(long)(i + 2*H) * PSY * PSZ"
                f" + (long)(jc + H) * PSZ + (kc + H)];")
            ring_shift.append(
                f"        for (int p = 0; p < 2*H; ++p)\n"
                f"            r_{nm}_{lin}[p] = r_{nm}_{lin}[p + 1];")

        body = cg.emit_statements(map_dict, tmp_instructions)
        params = self._declare_fields(cg, field_args, "real*")
        defines = geometry_defines(halo, rank_shape, rtype=_RTYPE[dtype])
        defines += (f"#define SBZ {sbz}\n#define SBY {sby}\n"
                    f"#define SXCHUNK {xchunk}\n")
        self._build(STENCIL_TEMPLATE.format(
            defines=defines, preamble=PREAMBLE, name=name, params=params,
            lds_decls="\n".join(lds_decls),
            stage="\n".join(stage),
            ring_init="\n".join(ring_init),
            ring_load="\n".join(ring_load),
            ring_shift="\n".join(ring_shift),
            body=body), name, compile)
        self._tiled((sbz, sby, xchunk), rank_shape)


def get_stencil_kernel(map_dict, tmp_instructions, field_args,
                       scalar_names, halo, rank_shape,
                       name="stencil_map", dtype=torch.float64):
    """LDS-staged stencil kernel, falling back to the plain elementwise
    form when no prefetchable reads exist or LDS would overflow."""
    try:
        k = JitStencil(map_dict, tmp_instructions, field_args,
                       scalar_names, halo, rank_shape, name=name,
                       dtype=dtype)
        if k.lds_bytes > 0:
            return k
    except ValueError:
        pass
    return JitElementwise(map_dict, tmp_instructions, field_args,
                          scalar_names, halo, rank_shape, name=name,
                          dtype=dtype)


# ---------------------------------------------------------------------------
# JIT'd fused elementwise map + simultaneous reductions over the INPUT
# state (MI355X traffic optimization: the RK stage kernel reads f, dfdt
# and computes lap f inline anyway — accumulating the energy reducers in
# the same pass removes the standalone lap+reduction kernel from the hot
# loop entirely; see fusion.StencilRKStepper).

STAGERED_TEMPLATE = """{defines}
{preamble}
#define NRED {nred}
extern "C" __global__ __launch_bounds__(TBZ * TBY) void {name}(
    {params})
{{
    double acc[NRED];
    {init}
    const int k = blockIdx.x * TBZ + (threadIdx.x % TBZ);
    const int j = blockIdx.y * TBY + (threadIdx.x / TBZ);
    const int i0 = blockIdx.z * XCHUNK;
    const int i1 = (i0 + XCHUNK < NX) ? i0 + XCHUNK : NX;
    if (k < NZ && j < NY) {{
        for (int i = i0; i < i1; ++i) {{
            {body}
        }}
    }}
"""


class JitStageReduction(_PartialsKernel):
    """Fused per-site map + multi-quantity reduction of the pre-update
    state.  Emission order per site: temporaries (which include the
    inline Laplacian), reduction accumulation (reads input values), then
    the update stores — so the reducers see the input state even for
    in-place unknowns."""

    _dtype_error = _REDUCTION_DTYPE_ERROR

    def __init__(self, map_dict, tmp_instructions, entries, field_args,
                 scalar_names, halo, rank_shape, name="rk_stage_red",
                 tile=(64, 4, 64), compile=True):
        self.rank_shape = tuple(rank_shape)
        self.tile = tile
        self.dtype = torch.float64      # fp64-only kernel (double* params)
        self.entries = entries
        nred = len(entries)
        cg = Codegen(field_args, halo, rank_shape)

        lines = []
        for lhs, rhs in (tmp_instructions or {}).items():
            tname = lhs.name if hasattr(lhs, "name") else str(lhs)
            cg.tmp_names.add(tname)
            lines.append(f"const double {tname} = {cg.emit(rhs)};")
        init_lines, acc_lines, combine = _reducer_pieces(cg, entries)
        lines += acc_lines
        for lhs, rhs in map_dict.items():
            lines.append(f"{cg.emit(lhs)} = {cg.emit(rhs)};")

        params = self._declare_fields(cg, field_args, "double*",
                                      [self.PARTIALS])

        defines = geometry_defines(halo, rank_shape)
        defines += _tile_defines(tile)
        defines += combine
        self._build((STAGERED_TEMPLATE + REDUCTION_TAIL).format(
            defines=defines, preamble=PREAMBLE, nred=nred, name=name,
            params=params, init="\n    ".join(init_lines),
            body="\n            ".join(lines)), name, compile)
        self._tiled(tile, rank_shape)


def get_stage_reduction_kernel(map_dict, tmp_instructions, entries,
                               field_args, scalar_names, halo, rank_shape,
                               name="rk_stage_red", tile=(64, 4, 64)):
    return JitStageReduction(map_dict, tmp_instructions, entries,
                             field_args, scalar_names, halo, rank_shape,
                             name=name, tile=tile)


# ---------------------------------------------------------------------------
# Fused periodic-wrap kernel: all single-rank axes' halo faces in ONE
# launch (the torch slicing path costs ~6 kernel launches per field per
# stage).  Axes are wrapped concurrently, so edge/corner halos are NOT
# propagated — star-stencil contract, same as share_halos_start.

WRAP_TEMPLATE = """{defines}
extern "C" __global__ __launch_bounds__(256) void {name}(
    real* __restrict__ f)
{{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
#if WRAPX
    for (long t = tid; t < (long)NF * 2 * H * PSY * PSZ; t += stride) {{
        const int c = (int)(t % PSZ);
        long r = t / PSZ;
        const int j = (int)(r % PSY);
        r /= PSY;
        const int p = (int)(r % (2 * H));
        const long base = (r / (2 * H)) * PVOL;
        const int xd = p < H ? p : NX + H + (p - H);
        const int xs = p < H ? p + NX : p;
        f[base + ((long)xd * PSY + j) * PSZ + c] =
            f[base + ((long)xs * PSY + j) * PSZ + c];
    }}
#endif
#if WRAPY
    for (long t = tid; t < (long)NF * 2 * H * PSX * PSZ; t += stride) {{
        const int c = (int)(t % PSZ);
        long r = t / PSZ;
        const int i = (int)(r % PSX);
        r /= PSX;
        const int p = (int)(r % (2 * H));
        const long base = (r / (2 * H)) * PVOL;
        const int yd = p < H ? p : NY + H + (p - H);
        const int ys = p < H ? p + NY : p;
        f[base + ((long)i * PSY + yd) * PSZ + c] =
            f[base + ((long)i * PSY + ys) * PSZ + c];
    }}
#endif
#if WRAPZ
    for (long t = tid; t < (long)NF * 2 * H * PSX * PSY; t += stride) {{
        long r = t;
        const int j = (int)(r % PSY);
        r /= PSY;
        const int i = (int)(r % PSX);
        r /= PSX;
        const int p = (int)(r % (2 * H));
        const long base = (r / (2 * H)) * PVOL;
        const int zd = p < H ? p : NZ + H + (p - H);
        const int zs = p < H ? p + NZ : p;
        f[base + ((long)i * PSY + j) * PSZ + zd] =
            f[base + ((long)i * PSY + j) * PSZ + zs];
    }}
#endif
}}
"""

_wrap_cache = {}


def wrap_source(rank_shape, h, nf, wrap_axes, dtype):
    """(kernel name, HIP source) of the wrap of ``wrap_axes`` of ``nf``
    arrays of ``dtype`` with interior ``rank_shape`` and halo ``h``.
    Needs no device."""
    defines = geometry_defines(h, rank_shape, rtype=_RTYPE[dtype])
    defines += f"#define NF {nf}\n"
    for ax, nm in enumerate("XYZ"):
        defines += f"#define WRAP{nm} {1 if ax in wrap_axes else 0}\n"
    name = _wrap_name(h, nf, wrap_axes)
    return name, WRAP_TEMPLATE.format(defines=defines, name=name)


def _wrap_name(h, nf, wrap_axes):
    return f"wrap_star_{h}_{nf}_" + "".join(
        str(int(ax in wrap_axes)) for ax in range(3))


def wrap_star(fx, halo, wrap_axes):
    """Periodic wrap of all ``wrap_axes`` halo faces of ``fx`` in one
    kernel launch (star-stencil contract; see WRAP_TEMPLATE)."""
    h = max(halo) if isinstance(halo, (tuple, list)) else halo
    nxp, nyp, nzp = fx.shape[-3:]
    rank_shape = (nxp - 2 * h, nyp - 2 * h, nzp - 2 * h)
    nf = 1
    for n in fx.shape[:-3]:
        nf *= n
    kid = _cached_kernel(
        _wrap_cache, (rank_shape, h, nf, tuple(sorted(wrap_axes)), fx.dtype),
        _wrap_name(h, nf, wrap_axes),
        lambda: wrap_source(rank_shape, h, nf, wrap_axes, fx.dtype)[1])
    _check_tensor("f", fx)
    cells = max((nxp + 2 * h) * (nyp + 2 * h), 1) * 2 * h * nf
    _launch_1d(kid, cells, [fx.data_ptr()], cap=4096)


# ---------------------------------------------------------------------------
# JIT'd simultaneous reductions

# Written once for every kernel that leaves per-block partials: ``{bid}``
# declares the block's flat column ``bid`` in the partials buffer and
# ``{stride}`` is that buffer's row length.
PARTIALS_TAIL = """
    __shared__ double sd[TBZ * TBY];
    {bid}
    for (int r = 0; r < NRED; ++r) {{
        sd[threadIdx.x] = acc[r];
        __syncthreads();
        for (int s = (TBZ * TBY) / 2; s > 0; s >>= 1) {{
            if ((int)threadIdx.x < s)
                sd[threadIdx.x] = COMBINE(r, sd[threadIdx.x],
                                          sd[threadIdx.x + s]);
            __syncthreads();
        }}
        if (threadIdx.x == 0)
            partials[(long)r * {stride} + bid] = sd[0];
        __syncthreads();
    }}
}}
"""

# a launch that owns its partials buffer: one column per block of its grid
_GRID_BID = """const int nblk = gridDim.x * gridDim.y * gridDim.z;
    const int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x
                    + blockIdx.x;"""

REDUCTION_TAIL = PARTIALS_TAIL.replace("{bid}", _GRID_BID).replace(
    "{stride}", "nblk")

REDUCTION_TEMPLATE = """{defines}
{preamble}
#define NRED {nred}
extern "C" __global__ __launch_bounds__(TBZ * TBY) void {name}(
    {params})
{{
    double acc[NRED];
    {init}
    const int k = blockIdx.x * TBZ + (threadIdx.x % TBZ);
    const int j = blockIdx.y * TBY + (threadIdx.x / TBZ);
    const int i0 = blockIdx.z * XCHUNK;
    const int i1 = (i0 + XCHUNK < NX) ? i0 + XCHUNK : NX;
    if (k < NZ && j < NY) {{
        for (int i = i0; i < i1; ++i) {{
            {body}
        }}
    }}
""" + REDUCTION_TAIL

_OP_INIT = {"sum": "0.0", "avg": "0.0", "prod": "1.0",
            "max": "-1.0e308", "min": "1.0e308"}
_OP_COMBINE = {"sum": "(a + b)", "avg": "(a + b)", "prod": "(a * b)",
               "max": "fmax(a, b)", "min": "fmin(a, b)"}


def _reducer_pieces(cg, entries, wide_scalars=False):
    """(``acc[]`` init lines, per-site accumulate lines, the ``COMBINE``
    define) of ``entries``.  The per-site values are emitted through
    ``cg`` here, so the call's place among the caller's other emissions
    fixes the reducers' place in the kernel's scalar parameter order.
    ``wide_scalars`` brackets each value for a :class:`_LapCodegen`
    (see there)."""
    init_lines, acc_lines, combine_cases = [], [], []
    for r, (expr, op) in enumerate(entries):
        comb = _OP_COMBINE[op]
        init_lines.append(f"acc[{r}] = {_OP_INIT[op]};")
        if wide_scalars:
            cg.wide_scalars = True
        val = cg.emit(expr)
        if wide_scalars:
            cg.wide_scalars = False
        acc_lines.append(
            "{ const double a = acc[%d]; const double b = %s; "
            "acc[%d] = %s; }" % (r, val, r, comb))
        combine_cases.append(f"(r == {r}) ? {comb} : ")
    combine = "".join(combine_cases) + "0.0"
    return (init_lines, acc_lines,
            f"#define COMBINE(r, a, b) ({combine})\n")


class JitReduction(_PartialsKernel):
    """Fused multi-quantity grid reduction → per-block partials,
    finished with torch ops + one packed allreduce by the caller."""

    _dtype_error = _REDUCTION_DTYPE_ERROR

    def __init__(self, entries, field_args, scalar_names, halo, rank_shape,
                 name="reduce_map", tile=(64, 4, 64), dtype=None,
                 compile=True):
        dtype = dtype if dtype is not None else torch.float64
        self.rank_shape = tuple(rank_shape)
        self.tile = tile
        self.dtype = dtype
        self.entries = entries
        nred = len(entries)
        cg = Codegen(field_args, halo, rank_shape)

        init_lines, body_lines, combine = _reducer_pieces(cg, entries)
        params = self._declare_fields(cg, field_args, "const real*",
                                      [self.PARTIALS])

        defines = geometry_defines(halo, rank_shape, rtype=_RTYPE[dtype])
        defines += _tile_defines(tile)
        defines += combine
        self._build(REDUCTION_TEMPLATE.format(
            defines=defines, preamble=PREAMBLE, nred=nred, name=name,
            params=params,
            init="\n    ".join(init_lines),
            body="\n        ".join(body_lines)), name, compile)
        self._tiled(tile, rank_shape)


def get_reduction_kernel(entries, field_args, scalar_names, halo,
                         rank_shape, tile=(64, 4, 64), dtype=None):
    return JitReduction(entries, field_args, scalar_names, halo,
                        rank_shape, tile=tile, dtype=dtype)


# ---------------------------------------------------------------------------
# JIT'd histogrammer: LDS bins + device-scope atomic merge

HISTOGRAM_TEMPLATE = """{defines}
{preamble}
#define NHIST {nhist}
#define NBINS {nbins}
extern "C" __global__ __launch_bounds__(256) void {name}(
    {params})
{{
    __shared__ double lh[NHIST * NBINS];
    for (int b = threadIdx.x; b < NHIST * NBINS; b += blockDim.x)
        lh[b] = 0.0;
    __syncthreads();

    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)NX * NY * NZ;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; idx < total; idx += stride) {{
        const int k = (int)(idx % NZ);
        const long t = idx / NZ;
        const int j = (int)(t % NY);
        const int i = (int)(t / NY);
        {body}
    }}
    __syncthreads();
    for (int b = threadIdx.x; b < NHIST * NBINS; b += blockDim.x)
        atomicAdd(&hist[b], lh[b]);
}}
"""


# Large-bin-count fallback: accumulate straight into global memory
# (device-scope atomics) when NHIST*NBINS doubles exceed the LDS
# budget of one workgroup (the reference caps the workgroup and merges
# through global atomics too: histogram.py:69,114-163).
HISTOGRAM_GLOBAL_TEMPLATE = """{defines}
{preamble}
#define NHIST {nhist}
#define NBINS {nbins}
extern "C" __global__ __launch_bounds__(256) void {name}(
    {params})
{{
    double* lh = hist;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)NX * NY * NZ;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; idx < total; idx += stride) {{
        const int k = (int)(idx % NZ);
        const long t = idx / NZ;
        const int j = (int)(t % NY);
        const int i = (int)(t / NY);
        {body}
    }}
}}
"""

# one workgroup may use at most 64 KB LDS on gfx9xx
_HIST_LDS_DOUBLES = 8192


class JitHistogram(_JitKernel):
    """Simultaneous weighted histograms of fp64 or fp32 fields (``using
    real = double|float``).  Bin values and weights are evaluated in
    the fields' type; each weight is widened to double where it is
    added, and the bins stay float64 whatever the fields are.
    ``compile=False`` only generates ``self.source``."""

    block = 256
    _dtype_error = ("histogram argument '{name}' has dtype {got}, kernel "
                    "compiled for {want}")

    def __init__(self, pairs, num_bins, field_args, scalar_names, halo,
                 rank_shape, name="hist_map", dtype=None, compile=True):
        dtype = dtype if dtype is not None else torch.float64
        self.rank_shape = tuple(rank_shape)
        self.num_bins = num_bins
        self.nhist = len(pairs)
        self.dtype = dtype
        cg = Codegen(field_args, halo, rank_shape)
        body = []
        for hh, (bin_expr, weight_expr) in enumerate(pairs):
            b = cg.emit(bin_expr)
            w = cg.emit(weight_expr)
            body.append(
                "{ int bb = (int)(%s); bb = bb < 0 ? 0 : "
                "(bb >= NBINS ? NBINS - 1 : bb); "
                "atomicAdd(&lh[%d * NBINS + bb], (double)(%s)); }"
                % (b, hh, w))
        params = self._declare_fields(cg, field_args, "const real*",
                                      ["double* __restrict__ hist"])
        template = (HISTOGRAM_TEMPLATE
                    if self.nhist * num_bins <= _HIST_LDS_DOUBLES
                    else HISTOGRAM_GLOBAL_TEMPLATE)
        self._build(template.format(
            defines=geometry_defines(halo, rank_shape,
                                     rtype=_RTYPE[dtype]),
            preamble=PREAMBLE,
            nhist=self.nhist, nbins=num_bins, name=name, params=params,
            body="\n        ".join(body)), name, compile)
        self.grid = _blocks_1d(int(np.prod(rank_shape)), 1024)

    def __call__(self, env):
        ptrs, dev = self._pointers(env)
        hist = torch.zeros((self.nhist, self.num_bins),
                           dtype=torch.float64, device=dev)
        self._launch(self.key, (self.grid, 1, 1), env,
                     ptrs + [hist.data_ptr()])
        return hist.cpu().numpy()


def get_histogram_kernel(pairs, num_bins, field_args, scalar_names, halo,
                         rank_shape, dtype=None):
    return JitHistogram(pairs, num_bins, field_args, scalar_names, halo,
                        rank_shape, dtype=dtype)


# ---------------------------------------------------------------------------
# Spectra binning: LDS per-block bins + one global merge.  torch's
# index_add_ funnels every site's atomic into ~500 global bins and
# takes seconds at 512^3; this kernel does it in milliseconds
# (reference K11, spectra.py:103-138).

SPECTRA_BIN_SRC = """
#define NBINS {nbins}
extern "C" __global__ __launch_bounds__(256) void {name}(
    const {fk_t}* __restrict__ fk, const double* __restrict__ wbase,
    const int* __restrict__ bidx, double* __restrict__ hist, int n)
{{
    __shared__ double lh[NBINS];
    for (int b = threadIdx.x; b < NBINS; b += 256) lh[b] = 0.0;
    __syncthreads();
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {{
        {load}
        atomicAdd(&lh[bidx[i]], wbase[i] * (re * re + im * im));
    }}
    __syncthreads();
    for (int b = threadIdx.x; b < NBINS; b += 256)
        atomicAdd(&hist[b], lh[b]);
}}
"""

# storage type -> (kernel name, fk element type, the load of one mode).
# A complex64 mode moves as one 8-byte access and is widened on load;
# |f|^2, the weights and the bins are double for either storage type.
_SPECTRA_BIN_FORMS = {
    "complex128": ("spectra_bin", "double",
                   "const double re = fk[2 * i];\n"
                   "        const double im = fk[2 * i + 1];"),
    "complex64": ("spectra_bin_c64", "float2",
                  "const float2 v = fk[i];\n"
                  "        const double re = (double)v.x;\n"
                  "        const double im = (double)v.y;"),
}
_CTYPE_NAMES = {torch.complex128: "complex128", torch.complex64: "complex64",
                "complex128": "complex128", "complex64": "complex64"}


def _ctype_name(ctype):
    try:
        return _CTYPE_NAMES[ctype]
    except (KeyError, TypeError):
        raise ValueError(f"ctype must be complex128 or complex64, "
                         f"got {ctype!r}") from None


def spectra_bin_source(num_bins, ctype="complex128"):
    """HIP source of the binning kernel for ``num_bins`` bins and modes
    stored as ``ctype``.  Needs no device."""
    name, fk_t, load = _SPECTRA_BIN_FORMS[_ctype_name(ctype)]
    return SPECTRA_BIN_SRC.format(nbins=int(num_bins), name=name, fk_t=fk_t,
                                  load=load)


_spectra_bin_cache = {}


def _spectra_bin(fk, wbase, bidx, num_bins, ctype):
    _check_arg("fk", fk, getattr(torch, ctype),
               f"; this binning kernel takes {ctype}")
    n = fk.numel()
    for name, t, dtype in (("wbase", wbase, torch.float64),
                           ("bidx", bidx, torch.int32)):
        _check_arg(name, t, dtype, f", expected {dtype}",
                   numel=(n, "fk has"))
    # the complex128 key is the bare bin count, as it always was
    kid = _cached_kernel(
        _spectra_bin_cache,
        num_bins if ctype == "complex128" else (num_bins, ctype),
        _SPECTRA_BIN_FORMS[ctype][0],
        lambda: spectra_bin_source(num_bins, ctype))
    hist = torch.zeros(num_bins, dtype=torch.float64, device=fk.device)
    _launch_1d(kid, n, [fk.data_ptr(), wbase.data_ptr(), bidx.data_ptr(),
                        hist.data_ptr()], [n], cap=4096)
    return hist


def spectra_bin(fk, wbase, bidx, num_bins):
    """|f_k|²-weighted LDS-binned histogram; fk complex128, wbase fp64,
    bidx int32 (all flat, same length).  Returns fp64 hist[num_bins]."""
    return _spectra_bin(fk, wbase, bidx, num_bins, "complex128")


def spectra_bin_c64(fk, wbase, bidx, num_bins):
    """:func:`spectra_bin` for complex64 modes: one 8-byte load per mode,
    widened once; the sum and ``hist`` are fp64 as there."""
    return _spectra_bin(fk, wbase, bidx, num_bins, "complex64")


# ---------------------------------------------------------------------------
# fused k-space projector kernels: one launch per operation, ε-basis
# built in registers (reference pystella/fourier/projectors.py:108-236
# runs each of these as ONE generated kernel too; round 1 shipped them
# as multi-launch torch chains — these close K10).  The storage type of
# the modes is a generation-time choice (complex128, or complex64 for the
# objects built on a float32 transform); the bodies are the same.

PROJECTOR_PREAMBLE = """
struct cplx { double x; double y; };
__device__ inline cplx cmul(cplx a, cplx b)
{ return {a.x*b.x - a.y*b.y, a.x*b.y + a.y*b.x}; }
__device__ inline cplx cadd(cplx a, cplx b)
{ return {a.x + b.x, a.y + b.y}; }
__device__ inline cplx conjg(cplx a) { return {a.x, -a.y}; }
__device__ inline cplx cscale(double s, cplx a)
{ return {s * a.x, s * a.y}; }
%LDST%"""

# how a mode is loaded and stored, per storage type (the %LDST% of
# PROJECTOR_PREAMBLE) with the element type of the data pointers.
# complex64 moves as one float2 access, widened once on the load and
# rounded once on the store; cplx and all arithmetic stay double.
_PROJECTOR_LDST = {
    "complex128": ("double", """\
#define LDC(p, c) cplx{ (p)[2*((long)(c)*VOLK + idx)], \\
                        (p)[2*((long)(c)*VOLK + idx) + 1] }
#define STC(p, c, v) { (p)[2*((long)(c)*VOLK + idx)] = (v).x; \\
                       (p)[2*((long)(c)*VOLK + idx) + 1] = (v).y; }
"""),
    "complex64": ("float2", """\
__device__ inline cplx widen(const float2 v)
{ return {(double)v.x, (double)v.y}; }
#define LDC(p, c) widen((p)[(long)(c)*VOLK + idx])
#define STC(p, c, v) { (p)[(long)(c)*VOLK + idx] = \\
                           make_float2((float)(v).x, (float)(v).y); }
"""),
}

PROJECTOR_KERNEL = """
extern "C" __global__ __launch_bounds__(256) void {name}(
    {params},
    const double* __restrict__ eff_x,
    const double* __restrict__ eff_y,
    const double* __restrict__ eff_z)
{{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= VOLK) return;
    const int kk = (int)(idx % NKZ);
    const int jj = (int)((idx / NKZ) % NKY);
    const int ii = (int)(idx / ((long)NKZ * NKY));
    const double kx = eff_x[ii], ky = eff_y[jj], kz = eff_z[kk];
    const double ksq = kx*kx + ky*ky + kz*kz;
    const bool kzero = (fabs(kx) < 1e-14) && (fabs(ky) < 1e-14)
                        && (fabs(kz) < 1e-14);
    (void)ksq; (void)kzero;
    {eps}
    {body}
}}
"""

# ε-basis construction, matching the torch construction in
# pystella_amd/fourier/projectors.py:57-78 (reference
# projectors.py:123-142 incl. the k_x = k_y = 0 special case)
PROJECTOR_EPS = """
    const double Kappa = sqrt(kx*kx + ky*ky);
    const double kmag = sqrt(ksq);
    const double kmag_s = (kmag > 0.) ? kmag : 1.0;
    const double Kappa_s = (Kappa > 0.) ? Kappa : 1.0;
    const bool kxy0 = (fabs(kx) < 1e-10) && (fabs(ky) < 1e-10);
    const bool kznz = fabs(kz) > 1e-10;
    const double S2 = 0.7071067811865476;
    cplx eps0, eps1, eps2;
    if (kxy0) {
        eps0 = kznz ? cplx{S2, 0.} : cplx{0., 0.};
        eps1 = kznz ? cplx{0., S2} : cplx{0., 0.};
        eps2 = cplx{0., 0.};
    } else {
        eps0 = cplx{ kx*kz/kmag_s/Kappa_s*S2, -ky/Kappa_s*S2 };
        eps1 = cplx{ ky*kz/kmag_s/Kappa_s*S2,  kx/Kappa_s*S2 };
        eps2 = cplx{ -Kappa/kmag_s*S2, 0. };
    }
    (void)eps0; (void)eps1; (void)eps2;
"""


def _proj_sym(c, d):
    """tid(c,d) for 1-based (c,d) -> symmetric 6-component index."""
    a, b = min(c, d), max(c, d)
    return {(1, 1): 0, (1, 2): 1, (1, 3): 2,
            (2, 2): 3, (2, 3): 4, (3, 3): 5}[(a, b)]


def _projector_bodies():
    eps = ["eps0", "eps1", "eps2"]
    bodies = {}

    bodies["transversify"] = ("""
    cplx v0 = LDC(vec,0), v1 = LDC(vec,1), v2 = LDC(vec,2);
    const double iksq = (ksq > 0.) ? 1.0 / ksq : 0.0;
    cplx div = cadd(cadd(cscale(kx,v0), cscale(ky,v1)), cscale(kz,v2));
    cplx r0 = {v0.x - kx*iksq*div.x, v0.y - kx*iksq*div.y};
    cplx r1 = {v1.x - ky*iksq*div.x, v1.y - ky*iksq*div.y};
    cplx r2 = {v2.x - kz*iksq*div.x, v2.y - kz*iksq*div.y};
    if (kzero) { r0 = {0.,0.}; r1 = {0.,0.}; r2 = {0.,0.}; }
    STC(out,0,r0) STC(out,1,r1) STC(out,2,r2)
""", ["vec", "out"], False)

    pm_sum = "".join(
        f"""
    p = cadd(p, cmul(v{m}, conjg({eps[m]})));
    mi = cadd(mi, cmul(v{m}, {eps[m]}));""" for m in range(3))
    bodies["vec_to_pol"] = ("""
    cplx v0 = LDC(vec,0), v1 = LDC(vec,1), v2 = LDC(vec,2);
    cplx p = {0.,0.}, mi = {0.,0.};""" + pm_sum + """
    STC(plus,0,p) STC(minus,0,mi)
""", ["vec", "plus", "minus"], True)

    p2v = "".join(
        f"""
    cplx r{m} = cadd(cmul(p, {eps[m]}), cmul(mi, conjg({eps[m]})));"""
        for m in range(3))
    stores = " ".join(f"STC(out,{m},r{m})" for m in range(3))
    bodies["pol_to_vec"] = ("""
    cplx p = LDC(plus,0), mi = LDC(minus,0);""" + p2v + f"""
    {stores}
""", ["plus", "minus", "out"], True)

    bodies["decompose_vector"] = ("""
    cplx v0 = LDC(vec,0), v1 = LDC(vec,1), v2 = LDC(vec,2);
    cplx p = {0.,0.}, mi = {0.,0.};""" + pm_sum + """
    cplx div = cadd(cadd(cscale(kx,v0), cscale(ky,v1)), cscale(kz,v2));
    const double denom = (ksq > 0.) ? (TIMES_ABS_K ? sqrt(ksq) : ksq)
                                     : 1.0;
    cplx lng = { div.y / denom, -div.x / denom };
    if (kzero) lng = {0., 0.};
    STC(plus,0,p) STC(minus,0,mi) STC(lngp,0,lng)
""", ["vec", "plus", "minus", "lngp"], True)

    d2v = "".join(f"""
    cplx r{m} = cadd(cmul(p, {eps[m]}), cmul(mi, conjg({eps[m]})));
    {{ const double km = {"kx" if m == 0 else ("ky" if m == 1 else "kz")};
       const double fac = TIMES_ABS_K ? km : km / kmag_s;
       cplx extra = {{ -fac * lng.y, fac * lng.x }};
       if (!kzero) r{m} = cadd(r{m}, extra); }}""" for m in range(3))
    bodies["decomp_to_vec"] = ("""
    cplx p = LDC(plus,0), mi = LDC(minus,0), lng = LDC(lngp,0);"""
        + d2v + f"""
    {stores}
""", ["plus", "minus", "lngp", "out"], True)

    t2p_terms = "".join(
        f"""
    p = cadd(p, cmul(h{_proj_sym(c, d)},
                     cmul(conjg({eps[c-1]}), conjg({eps[d-1]}))));
    mi = cadd(mi, cmul(h{_proj_sym(c, d)},
                       cmul({eps[c-1]}, {eps[d-1]})));"""
        for c in range(1, 4) for d in range(1, 4))
    loads6 = " ".join(f"cplx h{m} = LDC(hij,{m});" for m in range(6))
    bodies["tensor_to_pol"] = (f"""
    {loads6}
    cplx p = {{0.,0.}}, mi = {{0.,0.}};""" + t2p_terms + """
    STC(plus,0,p) STC(minus,0,mi)
""", ["hij", "plus", "minus"], True)

    p2t = "".join(
        f"""
    cplx r{_proj_sym(a, b)} = cadd(
        cmul(p, cmul({eps[a-1]}, {eps[b-1]})),
        cmul(mi, cmul(conjg({eps[a-1]}), conjg({eps[b-1]}))));"""
        for a in range(1, 4) for b in range(a, 4))
    stores6 = " ".join(f"STC(hij,{m},r{m})" for m in range(6))
    bodies["pol_to_tensor"] = ("""
    cplx p = LDC(plus,0), mi = LDC(minus,0);""" + p2t + f"""
    {stores6}
""", ["plus", "minus", "hij"], True)

    return bodies


_PROJ_BODIES = _projector_bodies()
_proj_cache = {}


def _proj_kernel_name(op, ctype):
    return f"proj_{op}" + ("_c64" if ctype == "complex64" else "")


def projector_source(op, kshape, times_abs_k=False, ctype="complex128"):
    """HIP source of projector kernel ``op``; ``ctype`` is the storage
    type of every data pointer.  Needs no device."""
    body, names, needs_eps = _PROJ_BODIES[op]
    ctype = _ctype_name(ctype)
    elem, ldst = _PROJECTOR_LDST[ctype]
    params = ",\n    ".join(f"{elem}* __restrict__ {n}" for n in names)
    head = (f"#define TIMES_ABS_K {1 if times_abs_k else 0}\n"
            + _kshape_defines(kshape))
    return (head + PROJECTOR_PREAMBLE.replace("%LDST%", ldst)
            + PROJECTOR_KERNEL.format(
                name=_proj_kernel_name(op, ctype), params=params,
                eps=PROJECTOR_EPS if needs_eps else "", body=body))


def _projector_launch(op, kshape, ptrs, eff, times_abs_k, ctype):
    # the complex128 key is the one it always was
    key = (op, tuple(kshape), bool(times_abs_k))
    if ctype != "complex128":
        key += (ctype,)
    kid = _cached_kernel(
        _proj_cache, key, _proj_kernel_name(op, ctype),
        lambda: projector_source(op, kshape, times_abs_k, ctype))
    _launch_1d(kid, int(np.prod(kshape)),
               list(ptrs) + [e.data_ptr() for e in eff])


def projector_op(op, kshape, ptrs, eff, times_abs_k=False):
    """Launch fused projector kernel ``op`` over k-space ``kshape``.

    :arg ptrs: list of data_ptrs in the op's parameter order.
    :arg eff: (eff_x, eff_y, eff_z) contiguous fp64 device tensors.
    """
    _projector_launch(op, kshape, ptrs, eff, times_abs_k, "complex128")


def _c64_tensor(name, t, shape):
    _check_arg(name, t, torch.complex64,
               "; the complex64 observable kernels take complex64", shape)


def _c64_tables(eff, kshape):
    if len(eff) != 3:
        raise ValueError("eff has three entries")
    for ax, e, n in zip("xyz", eff, kshape):
        _kspace_table(f"eff_{ax}", e, n)


# leading component counts of each op's tensors, in parameter order
_PROJ_LEADING = {
    "transversify": (3, 3), "vec_to_pol": (3, 0, 0),
    "pol_to_vec": (0, 0, 3), "decompose_vector": (3, 0, 0, 0),
    "decomp_to_vec": (0, 0, 0, 3), "tensor_to_pol": (6, 0, 0),
    "pol_to_tensor": (0, 0, 6)}


def projector_op_c64(op, kshape, tensors, eff, times_abs_k=False):
    """:func:`projector_op` for complex64 modes.  Takes the tensors
    themselves, in the op's parameter order, and checks them: contiguous
    complex64 device tensors of ``(ncomp,) + kshape`` (``kshape`` alone
    for a scalar), outputs possibly views of the input as in
    :func:`projector_op`.  ``eff`` stays fp64."""
    if op not in _PROJ_LEADING:
        raise ValueError(f"unknown projector op {op!r}")
    kshape = tuple(int(n) for n in kshape)
    lead = _PROJ_LEADING[op]
    if len(tensors) != len(lead):
        raise ValueError(f"{op} takes {len(lead)} tensors, "
                         f"got {len(tensors)}")
    for i, (t, nc) in enumerate(zip(tensors, lead)):
        _c64_tensor(f"tensors[{i}]", t,
                    ((nc,) if nc else ()) + kshape)
    _c64_tables(eff, kshape)
    if int(np.prod(kshape)) == 0:
        return
    _projector_launch(op, kshape, [t.data_ptr() for t in tensors], eff,
                      times_abs_k, "complex64")


def tt_project_c64(hij, out, eff, kshape):
    """Transverse-traceless projection of a complex64 ``hij`` of shape
    ``(6,) + kshape`` into ``out`` (which may be ``hij``) on the f64
    matrix cores: 8-byte loads widened to double, one rounded 8-byte
    store (csrc/tt_mfma.hip)."""
    kshape = tuple(int(n) for n in kshape)
    _c64_tensor("hij", hij, (6,) + kshape)
    _c64_tensor("out", out, (6,) + kshape)
    _c64_tables(eff, kshape)
    vol = int(np.prod(kshape))
    if vol == 0:
        return
    ext().tt_project_c64(hij.data_ptr(), out.data_ptr(),
                         eff[0].data_ptr(), eff[1].data_ptr(),
                         eff[2].data_ptr(), kshape[1], kshape[2], vol,
                         _stream())


# ---------------------------------------------------------------------------
# fused k-space kernels of SpectralCollocator and SpectralPoissonSolver:
# one launch per operation, fk read once, no k-space temporaries
# (reference pystella/fourier/derivs.py:93-108 and poisson.py:96-101
# run each as ONE generated kernel; these close K13 and K14).  Complex
# values move as one 16-byte access per mode (8 bytes in the complex64
# forms, whose arithmetic is the same doubles).  Every product that is
# then added goes through rounded(): the JIT compiles with
# -ffp-contract=fast, which fuses even under a contract(off) pragma, and
# a fused multiply-add is not the torch chain's result.  The empty asm
# emits nothing; it only hides the product from the contraction.

KSPACE_KERNEL = """
__device__ inline double rounded(double x)
{{ asm("" : "+v"(x)); return x; }}

extern "C" __global__ __launch_bounds__(256) void {name}(
    {params})
{{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= VOLK) return;
    const int kk = (int)(idx % NKZ);
    const int jj = (int)((idx / NKZ) % NKY);
    const int ii = (int)(idx / ((long)NKZ * NKY));
    (void)ii; (void)jj; (void)kk;
    {body}
}}
"""

KSPACE_DERIV_OUTS = ("pdx", "pdy", "pdz", "lap")


class _KspaceModes:
    """How a kernel declares, loads and stores its modes.  The complex64
    form differs from the complex128 one in nothing else: a stored mode
    is one 8-byte access, widened to double on the load; every
    expression is the complex128 form's, in double; a result is rounded
    once, in the ``make_float2`` of its 8-byte store."""

    def __init__(self, ctype):
        self.c64 = ctype == "complex64"
        self.elem = "float2" if self.c64 else "double2"

    def load(self, name, ptr):
        """Lines defining the ``const double2 name`` read from ``ptr``."""
        if not self.c64:
            return [f"const double2 {name} = {ptr}[idx];"]
        return [f"const float2 {name}_s = {ptr}[idx];",
                f"const double2 {name} = make_double2((double){name}_s.x, "
                f"(double){name}_s.y);"]

    def store(self, ptr, re, im):
        """The line storing ``(re, im)``, two double expressions."""
        if not self.c64:
            return f"{ptr}[idx] = make_double2({re}, {im});"
        return f"{ptr}[idx] = make_float2((float)({re}), (float)({im}));"


def _kspace_derivs_pieces(outs, modes):
    params = [f"const {modes.elem}* __restrict__ fk"]
    params += [f"{modes.elem}* __restrict__ {o}" for o in outs]
    tables = [f"k1{'xyz'[mu]}" for mu in range(3) if f"pd{'xyz'[mu]}" in outs]
    if "lap" in outs:
        tables += ["k2x", "k2y", "k2z"]
    params += [f"const double* __restrict__ {t}" for t in tables]
    params.append("const double inv_n")
    body = modes.load("v", "fk") + [
        "const double2 t = make_double2(v.x * inv_n, v.y * inv_n);"]
    for mu, (ax, i) in enumerate(zip("xyz", ("ii", "jj", "kk"))):
        if f"pd{ax}" in outs:
            body += [f"const double q{ax} = k1{ax}[{i}];",
                     modes.store(f"pd{ax}", f"-q{ax} * t.y", f"q{ax} * t.x")]
    if "lap" in outs:
        body += ["const double kx = k2x[ii], ky = k2y[jj], kz = k2z[kk];",
                 "const double mk2 = -((rounded(kx * kx) + rounded(ky * ky))",
                 "                     + rounded(kz * kz));",
                 modes.store("lap", "mk2 * t.x", "mk2 * t.y")]
    return params, body


def _kspace_pieces(op, flags, modes):
    """(parameter list, body lines) of kernel ``op``; consumes ``flags``."""
    elem = modes.elem
    if op == "derivs":
        outs = flags.pop("outs", None)
        if not outs or set(outs) - set(KSPACE_DERIV_OUTS):
            raise ValueError(
                f"outs must be a non-empty subset of {KSPACE_DERIV_OUTS}, "
                f"got {outs!r}")
        outs = tuple(o for o in KSPACE_DERIV_OUTS if o in outs)
        params, body = _kspace_derivs_pieces(outs, modes)
    elif op == "div_accum":
        mu = int(flags.pop("mu"))
        accumulate = bool(flags.pop("accumulate"))
        if mu not in (0, 1, 2):
            raise ValueError(f"mu must be 0, 1 or 2, got {mu}")
        params = [f"const {elem}* __restrict__ fk",
                  f"{elem}* __restrict__ div_k",
                  "const double* __restrict__ k1", "const double inv_n"]
        body = modes.load("v", "fk") + [
            f"const double q = k1[{('ii', 'jj', 'kk')[mu]}];",
            "double2 term = make_double2((-q * v.y) * inv_n, "
            "(q * v.x) * inv_n);"]
        if accumulate:
            body += modes.load("d", "div_k") + [
                "term = make_double2(d.x + rounded(term.x), "
                "d.y + rounded(term.y));"]
        body.append(modes.store("div_k", "term.x", "term.y") if modes.c64
                    else "div_k[idx] = term;")
    elif op == "poisson":
        # sol may be rhok itself: no __restrict__ on either
        params = [f"const {elem}* rhok", f"{elem}* sol",
                  "const double* __restrict__ ex",
                  "const double* __restrict__ ey",
                  "const double* __restrict__ ez",
                  "const double inv_n", "const double m_squared"]
        body = ["const double mk2 = (ex[ii] + ey[jj]) + ez[kk];"]
        body += modes.load("v", "rhok") + [
            "const double den = mk2 - m_squared;",
            "const double2 r = (mk2 < 0.0)" if modes.c64
            else "sol[idx] = (mk2 < 0.0)",
            "    ? make_double2((v.x * inv_n) / den, "
            "(v.y * inv_n) / den)",
            "    : make_double2(0.0, 0.0);"]
        if modes.c64:
            body.append(modes.store("sol", "r.x", "r.y"))
    else:
        raise ValueError(f"unknown k-space op {op!r}")
    if flags:
        raise TypeError(f"unexpected flags for {op}: {sorted(flags)}")
    return params, body


def _kspace_kernel_name(op, ctype):
    return f"kspace_{op}" + ("_c64" if ctype == "complex64" else "")


def kspace_source(op, kshape, ctype="complex128", **flags):
    """HIP source of k-space kernel ``op`` (``"derivs"`` with
    ``outs=``, ``"div_accum"`` with ``mu=`` and ``accumulate=``,
    ``"poisson"``) over k-space ``kshape``; ``ctype`` is the storage
    type of the modes (tables and scalars are double either way).
    Needs no device."""
    ctype = _ctype_name(ctype)
    params, body = _kspace_pieces(op, dict(flags), _KspaceModes(ctype))
    return _kshape_defines(kshape) + KSPACE_KERNEL.format(
        name=_kspace_kernel_name(op, ctype), params=",\n    ".join(params),
        body="\n    ".join(body))


_kspace_cache = {}


def _kspace_complex(name, t, kshape=None, ctype="complex128"):
    """Check a mode array (3-D; of ``kshape`` if given); its shape."""
    kernels = "k-space" if ctype == "complex128" else f"{ctype} k-space"
    _check_arg(name, t, getattr(torch, ctype),
               f"; the {kernels} kernels take {ctype}", kshape,
               ndim=None if kshape else 3)
    return tuple(t.shape)


def _kspace_table(name, t, n):
    _check_arg(name, t, torch.float64, "; the k-space tables are float64",
               (n,))


def _kspace_launch(op, kshape, ctype, ptrs, doubles, **flags):
    """``flags`` as the entry points normalise them (``outs`` in
    KSPACE_DERIV_OUTS order, ``mu`` an int, ``accumulate`` a bool)."""
    kid = _cached_kernel(
        _kspace_cache, (op, kshape, ctype) + tuple(sorted(flags.items())),
        _kspace_kernel_name(op, ctype),
        lambda: kspace_source(op, kshape, ctype, **flags))
    vol = int(np.prod(kshape))
    if vol == 0:
        return
    _launch_1d(kid, vol, ptrs, doubles=doubles)


def _kspace_derivs(ctype, fk, outs, k1, k2, inv_n):
    if not isinstance(outs, dict) or not outs \
            or set(outs) - set(KSPACE_DERIV_OUTS):
        raise ValueError("outs must map a non-empty subset of "
                         f"{KSPACE_DERIV_OUTS} to tensors")
    kshape = _kspace_complex("fk", fk, ctype=ctype)
    names = tuple(o for o in KSPACE_DERIV_OUTS if o in outs)
    for o in names:
        _kspace_complex(o, outs[o], kshape, ctype)
        if outs[o].data_ptr() == fk.data_ptr():
            raise ValueError(f"output {o} aliases fk")
    if len({outs[o].data_ptr() for o in names}) != len(names):
        raise ValueError("outputs alias each other")
    for mu in range(3):
        _kspace_table(f"k1[{mu}]", k1[mu], kshape[mu])
        _kspace_table(f"k2[{mu}]", k2[mu], kshape[mu])
    ptrs = [fk.data_ptr()] + [outs[o].data_ptr() for o in names]
    ptrs += [k1[mu].data_ptr() for mu in range(3)
             if f"pd{'xyz'[mu]}" in names]
    if "lap" in names:
        ptrs += [k.data_ptr() for k in k2]
    _kspace_launch("derivs", kshape, ctype, ptrs, [float(inv_n)], outs=names)


def _kspace_div_accum(ctype, fk, div_k, k1_mu, mu, inv_n, accumulate):
    kshape = _kspace_complex("fk", fk, ctype=ctype)
    _kspace_complex("div_k", div_k, kshape, ctype)
    if mu not in (0, 1, 2):
        raise ValueError(f"mu must be 0, 1 or 2, got {mu}")
    _kspace_table("k1_mu", k1_mu, kshape[mu])
    if div_k.data_ptr() == fk.data_ptr():
        raise ValueError("output div_k aliases fk")
    _kspace_launch("div_accum", kshape, ctype,
                   [fk.data_ptr(), div_k.data_ptr(), k1_mu.data_ptr()],
                   [float(inv_n)], mu=mu, accumulate=bool(accumulate))


def _kspace_poisson(ctype, rhok, sol, ex, ey, ez, inv_n, m_squared):
    kshape = _kspace_complex("rhok", rhok, ctype=ctype)
    _kspace_complex("sol", sol, kshape, ctype)
    for name, t, n in zip(("ex", "ey", "ez"), (ex, ey, ez), kshape):
        _kspace_table(name, t, n)
    _kspace_launch("poisson", kshape, ctype,
                   [rhok.data_ptr(), sol.data_ptr(), ex.data_ptr(),
                    ey.data_ptr(), ez.data_ptr()],
                   [float(inv_n), float(m_squared)])


def kspace_derivs(fk, outs, k1, k2, inv_n):
    """One launch: read ``fk`` once, write the requested spectral
    derivatives of ``t = fk * inv_n``.

    :arg outs: dict mapping any non-empty subset of ``pdx``, ``pdy``,
        ``pdz`` (``i k1_mu t``) and ``lap`` (``-|k2|^2 t``) to contiguous
        complex128 device tensors of ``fk``'s shape; none may be ``fk``.
    :arg k1, k2: the three per-axis float64 tables, flat on the device.
    """
    _kspace_derivs("complex128", fk, outs, k1, k2, inv_n)


def kspace_div_accum(fk, div_k, k1_mu, mu, inv_n, accumulate):
    """One launch: ``term = (i k1_mu fk) * inv_n``, stored to ``div_k``
    (``accumulate=False``) or added to it.  ``div_k`` may not be ``fk``."""
    _kspace_div_accum("complex128", fk, div_k, k1_mu, mu, inv_n, accumulate)


def kspace_poisson(rhok, sol, ex, ey, ez, inv_n, m_squared):
    """One launch: ``sol = (rhok * inv_n) / (mk2 - m_squared)`` where
    ``mk2 = (ex[i] + ey[j]) + ez[k] < 0``, zero elsewhere (the k = 0 mode
    is dropped for every mass).  The operation is purely per mode, so
    ``sol`` may be the same tensor as ``rhok``.  ``m_squared`` is a
    run-time argument: a new mass compiles nothing."""
    _kspace_poisson("complex128", rhok, sol, ex, ey, ez, inv_n, m_squared)


# The complex64 twins: the same arguments and checks with complex64
# modes and float64 tables.  Each stored mode is widened once to double,
# the formulas above are evaluated in double in the same order, and each
# real component of a result is rounded once to float32 on its store.

def kspace_derivs_c64(fk, outs, k1, k2, inv_n):
    """:func:`kspace_derivs` on complex64 modes: every stored output is
    one float32 rounding of the double result."""
    _kspace_derivs("complex64", fk, outs, k1, k2, inv_n)


def kspace_div_accum_c64(fk, div_k, k1_mu, mu, inv_n, accumulate):
    """:func:`kspace_div_accum` on complex64 modes: the stored ``div_k``
    is one float32 rounding of the double term, or of the stored
    ``div_k``, widened, plus the double term."""
    _kspace_div_accum("complex64", fk, div_k, k1_mu, mu, inv_n, accumulate)


def kspace_poisson_c64(rhok, sol, ex, ey, ez, inv_n, m_squared):
    """:func:`kspace_poisson` on complex64 modes, in place or not."""
    _kspace_poisson("complex64", rhok, sol, ex, ey, ez, inv_n, m_squared)


# ---------------------------------------------------------------------------
# user-written k-space maps (``KSpaceMap``, closes K1's complex half):
# the launch shape of KSPACE_KERNEL (256 threads, one mode each, the
# k-shape baked in) around statements that backend/codegen.py's
# KspaceCodegen lowers.  Every pointer is typed by its tensor's dtype, so
# a complex128 mode is one 16-byte access and a complex64 mode one of 8;
# every loaded value is widened once to double, all arithmetic is double,
# and each real component is rounded once, on its store.  The index
# decode is emitted only for a map that reads a per-axis table, in 32-bit
# arithmetic while the volume allows it.  Nothing shields products from
# contraction here: a map's result is defined to a tolerance, not to the
# bits of a torch chain.

KSPACE_MAP_TEMPLATE = """{defines}using real = double;
{preamble}
extern "C" __global__ __launch_bounds__(256) void {name}(
    {params})
{{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= VOLK) return;
    {decode}{body}
}}
"""

_KSPACE_MAP_DECODE = {
    # fewer than 2^31 modes: the decode needs no 64-bit division
    True: ("const unsigned lin = (unsigned)idx;\n"
           "    const int kk = (int)(lin % NKZ);\n"
           "    const int jj = (int)((lin / NKZ) % NKY);\n"
           "    const int ii = (int)(lin / (NKZ * NKY));\n"
           "    (void)ii; (void)jj; (void)kk;\n    "),
    False: ("const int kk = (int)(idx % NKZ);\n"
            "    const int jj = (int)((idx / NKZ) % NKY);\n"
            "    const int ii = (int)(idx / ((long)NKZ * NKY));\n"
            "    (void)ii; (void)jj; (void)kk;\n    "),
}


def _kspace_map_dtype(name, dtype):
    """The key of KSPACE_DTYPES for a torch dtype or its name."""
    key = str(dtype).replace("torch.", "")
    if key not in KSPACE_DTYPES:
        raise TypeError(
            f"argument {name} has dtype {dtype}; a k-space map takes "
            f"{sorted(KSPACE_DTYPES)}")
    return key


class JitKspaceMap(_JitKernel):
    """A compiled complex k-space map over k-space ``kshape``.

    :arg field_args: the :class:`FieldArg`\\ s of the grid fields and the
        per-axis tables (``axis`` 0, 1 or 2); their order is the
        pointers'.
    :arg dtypes: ``{name: dtype}`` of every one of them, torch dtypes or
        their names.

    ``compile=False`` only generates ``self.source``.
    """

    block = 256
    _dtype_error = ("argument {name} has dtype {got}, kernel compiled for "
                    "{short}")

    def __init__(self, map_dict, tmp_instructions, field_args, dtypes,
                 kshape, name="kspace_map", compile=True):
        self.kshape = tuple(int(n) for n in kshape)
        self.field_args = _spatial(field_args)
        self.dtypes = {fa.name: _kspace_map_dtype(fa.name, dtypes[fa.name])
                       for fa in self.field_args}
        for fa in self.field_args:
            if fa.axis is not None and KSPACE_DTYPES[self.dtypes[fa.name]][1]:
                raise TypeError(f"axis table {fa.name} has dtype "
                                f"{self.dtypes[fa.name]}; tables are real")
        cg = KspaceCodegen(field_args, self.dtypes)
        body = cg.emit_statements(map_dict, tmp_instructions)

        def pointer(name):
            elem = KSPACE_DTYPES[self.dtypes[name]][0]
            # a stored array may be read too, under the one name
            return (f"{elem}* {name}" if name in cg.stored
                    else f"const {elem}* __restrict__ {name}")

        params = self._declare(cg, [fa.name for fa in self.field_args],
                               pointer, scalar="const double", sep=",\n    ")
        vol = int(np.prod(self.kshape))
        self.stored = frozenset(cg.stored)
        self.blocks = _blocks_1d(vol)
        self._build(KSPACE_MAP_TEMPLATE.format(
            defines=_kshape_defines(self.kshape),
            preamble=PREAMBLE + KSPACE_PREAMBLE, name=name, params=params,
            decode=_KSPACE_MAP_DECODE[vol < 2**31] if cg.uses_axes else "",
            body="\n    ".join(body)), name, compile)

    def _arg_dtype(self, name):
        return getattr(torch, self.dtypes[name])

    def __call__(self, env):
        """Launch on ``env``'s tensors, which the caller has checked
        against ``kshape`` and ``dtypes``."""
        ptrs, _ = self._pointers(env)
        for fa in self.field_args:
            want = int(np.prod(fa.outer_shape, dtype=np.int64)) \
                * int(np.prod(self.kshape)) if fa.axis is None \
                else self.kshape[fa.axis]
            if env[fa.name].numel() != want:
                raise ValueError(
                    f"argument {fa.name} has {env[fa.name].numel()} "
                    f"elements, the kernel addresses {want}")
        if self.blocks == 0:
            return
        self._launch(self.key, (self.blocks, 1, 1), env, ptrs)


# ---------------------------------------------------------------------------
# fused Rayleigh mode kernel (RayleighGenerator rng="philox", closes K12):
# from the Philox4x32-10 words to the stored mode in one launch, one
# thread per mode, no k-space temporaries.  The definition is
# fourier/philox.py's; the counter holds the *global* canonical mode
# index, so a thread draws its Hermitian partner's numbers itself and
# every layout stores the same realisation.  The ten rounds live in
# named scalars (a runtime-indexed array would go to scratch) and the
# high products are __umulhi.  sincospi(2u) needs no large-argument
# reduction.  All arithmetic is double; the value is rounded once, on
# its 16- or 8-byte store.

RAYLEIGH_KERNEL = """
typedef unsigned int u32;

#define PHILOX_ROUND(K0, K1) {{ \\
    const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0; \\
    const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2; \\
    c0 = hi1 ^ c1 ^ (K0); c1 = lo1; \\
    c2 = hi0 ^ c3 ^ (K1); c3 = lo0; }}

// z = amp * sqrt_power * exp(2 pi i u_phs) of counter (c0, c1, c2, c3)
__device__ inline double2 rayleigh_mode(u32 c0, u32 c1, u32 c2, u32 c3,
                                        const u32 k0, const u32 k1,
                                        const double sp)
{{
    PHILOX_ROUND(k0, k1)
    PHILOX_ROUND(k0 + 0x9E3779B9u, k1 + 0xBB67AE85u)
    PHILOX_ROUND(k0 + 0x3C6EF372u, k1 + 0x76CF5D0Au)
    PHILOX_ROUND(k0 + 0xDAA66D2Bu, k1 + 0x32370B8Fu)
    PHILOX_ROUND(k0 + 0x78DDE6E4u, k1 + 0xED9EBA14u)
    PHILOX_ROUND(k0 + 0x1715609Du, k1 + 0xA9066899u)
    PHILOX_ROUND(k0 + 0xB54CDA56u, k1 + 0x646E171Eu)
    PHILOX_ROUND(k0 + 0x5384540Fu, k1 + 0x1FD5C5A3u)
    PHILOX_ROUND(k0 + 0xF1BBCDC8u, k1 + 0xDB3D7428u)
    PHILOX_ROUND(k0 + 0x8FF34781u, k1 + 0x96A522ADu)
    // exact doubles in (0, 1]
    const double u_phs = (double)((((unsigned long long)(c2 >> 11) << 32)
                                   | c3) + 1ull) * 0x1p-53;
#if RANDOM
    const double u_amp = (double)((((unsigned long long)(c0 >> 11) << 32)
                                   | c1) + 1ull) * 0x1p-53;
    const double a = sqrt(-log(u_amp)) * sp;
#else
    const double a = sp;
#endif
    double s, c;
    sincospi(2.0 * u_phs, &s, &c);
    return make_double2(a * c, a * s);
}}

extern "C" __global__ __launch_bounds__(256) void {name}(
    {params})
{{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= VOLK) return;
    const int kk = (int)(idx % NKZ);
    const int jj = (int)((idx / NKZ) % NKY);
    const int ii = (int)(idx / ((long)NKZ * NKY));
    const int gx = gxs[ii], gy = gys[jj], gz = gzs[kk];
    int cx = gx, cy = gy;
    bool conj = false, self = false;
#if IS_REAL
    if (gz == 0 || (NZ % 2 == 0 && gz == NZ / 2)) {{
        const int px = (NX - gx) % NX, py = (NY - gy) % NY;
        self = (px == gx) && (py == gy);
        if (!(gx < px || (gx == px && gy <= py))) {{
            cx = px; cy = py; conj = true;
        }}
    }}
#endif
    const u32 k0 = (u32)seed_lo, k1 = (u32)seed_hi;
    const double sp = sqrt_power[idx];
    {body}
}}
"""

_RAYLEIGH_STORE = """{{
        const double im = self ? 0.0 : (conj ? -{v}.y : {v}.y);
        {out}[idx] = make_{ct}(({rt}){v}.x, ({rt})im);
    }}"""

_RAYLEIGH_CTYPES = {torch.complex128: ("double2", "double"),
                    torch.complex64: ("float2", "float"),
                    "complex128": ("double2", "double"),
                    "complex64": ("float2", "float")}


def rayleigh_source(kshape, grid_shape, *, wkb, is_real, random, ctype):
    """HIP source of the fused Rayleigh mode kernel over this rank's
    k-space ``kshape`` of the global ``grid_shape``.  ``wkb`` selects the
    (f_k, f'_k) pair, ``is_real`` the Hermitian planes of an r2c
    transform, ``random`` the Rayleigh amplitude (else 1), ``ctype``
    (``torch.complex128``/``complex64`` or their names) the stored
    type.  Needs no device."""
    try:
        ct, rt = _RAYLEIGH_CTYPES[ctype]
    except (KeyError, TypeError):
        raise ValueError(f"ctype must be complex128 or complex64, "
                         f"got {ctype!r}") from None
    if len(kshape) != 3 or len(grid_shape) != 3:
        raise ValueError("kshape and grid_shape are 3-tuples")
    wkb, is_real, random = bool(wkb), bool(is_real), bool(random)
    params = [f"{ct}* __restrict__ fk"]
    if wkb:
        params.append(f"{ct}* __restrict__ dfk")
    params.append("const double* __restrict__ sqrt_power")
    if wkb:
        params.append("const double* __restrict__ omega")
    params += [f"const int* __restrict__ {t}" for t in ("gxs", "gys", "gzs")]
    params += ["const int seed_lo", "const int seed_hi", "const int draw"]
    if wkb:
        params.append("const double hubble")
    mode = ("rayleigh_mode((u32)cx, (u32)cy, (u32)gz, 2u * (u32)draw + %du, "
            "k0, k1, sp)")
    if wkb:
        body = [
            f"const double2 L = {mode % 0};",
            f"const double2 R = {mode % 1};",
            "const double rs2 = 0.70710678118654752440;",
            "const double2 f = make_double2((L.x + R.x) * rs2, "
            "(L.y + R.y) * rs2);",
            "const double2 d = make_double2((L.x - R.x) * rs2, "
            "(L.y - R.y) * rs2);",
            "const double w = omega[idx];",
            "const double2 g = make_double2(-(w * d.y) - hubble * f.x, "
            "w * d.x - hubble * f.y);",
            _RAYLEIGH_STORE.format(v="f", out="fk", ct=ct, rt=rt),
            _RAYLEIGH_STORE.format(v="g", out="dfk", ct=ct, rt=rt)]
    else:
        body = [f"const double2 z = {mode % 0};",
                _RAYLEIGH_STORE.format(v="z", out="fk", ct=ct, rt=rt)]
    head = "".join(
        f"#define {n} {int(v)}\n" for n, v in zip(
            ("NKX", "NKY", "NKZ", "NX", "NY", "NZ", "WKB", "IS_REAL",
             "RANDOM"),
            tuple(kshape) + tuple(grid_shape) + (wkb, is_real, random)))
    head += (f"#define CTYPE {ct}\n"
             "#define VOLK ((long)NKX * NKY * NKZ)\n")
    return head + RAYLEIGH_KERNEL.format(
        name="rayleigh_modes", params=",\n    ".join(params),
        body="\n    ".join(body))


_rayleigh_cache = {}


def rayleigh_modes(fk, dfk, sqrt_power, omega, tables, grid_shape, seed,
                   draw, hubble=0., *, is_real, random=True):
    """One launch: fill ``fk`` (and, for the WKB pair, ``dfk``) with the
    modes that fourier/philox.py defines for ``(seed, draw)``.

    :arg fk, dfk: contiguous complex128 or complex64 device tensors of
        this rank's k-shape; ``dfk=None`` selects ``generate``, and then
        ``omega`` is None as well.
    :arg sqrt_power, omega: float64 device tensors of the same shape.
    :arg tables: three flat int32 device tensors, this rank's global
        mode indices along each axis.
    """
    from pystella_amd.fourier.philox import check_draw, check_seed
    wkb = dfk is not None
    _check_arg("fk", fk, (torch.complex128, torch.complex64),
               "; the Rayleigh kernel stores complex128 or complex64",
               ndim=3)
    kshape = tuple(fk.shape)
    if wkb:
        _check_arg("dfk", dfk, fk.dtype, f", fk has {fk.dtype}", kshape)
        if dfk.data_ptr() == fk.data_ptr() and fk.numel():
            raise ValueError("output dfk aliases fk")
    if (omega is not None) != wkb:
        raise ValueError("omega goes with dfk: pass both or neither")
    for name, t in (("sqrt_power", sqrt_power), ("omega", omega))[:1 + wkb]:
        _check_arg(name, t, torch.float64,
                   "; the Rayleigh kernel reads float64", kshape)
    if len(tables) != 3 or len(grid_shape) != 3:
        raise ValueError("tables and grid_shape have three entries")
    for ax, t, n in zip("xyz", tables, kshape):
        _check_arg(f"tables[{ax}]", t, torch.int32,
                   "; the index tables are int32", (n,))
    grid_shape = tuple(int(n) for n in grid_shape)
    if min(grid_shape) < 1 or max(grid_shape) >= 2**31:
        raise ValueError(f"grid_shape {grid_shape} is out of range")
    seed = check_seed(seed)
    draw = check_draw(draw)
    vol = int(np.prod(kshape))
    if vol == 0:
        return
    flags = dict(wkb=wkb, is_real=bool(is_real), random=bool(random),
                 ctype=fk.dtype)
    key = (kshape, grid_shape) + tuple(sorted(flags.items(),
                                              key=lambda kv: kv[0]))
    kid = _cached_kernel(
        _rayleigh_cache, key, "rayleigh_modes",
        lambda: rayleigh_source(kshape, grid_shape, **flags))

    def signed(w):
        return w - 2**32 if w >= 2**31 else w

    ptrs = [fk.data_ptr()] + ([dfk.data_ptr()] if wkb else [])
    ptrs.append(sqrt_power.data_ptr())
    if wkb:
        ptrs.append(omega.data_ptr())
    ptrs += [t.data_ptr() for t in tables]
    _launch_1d(kid, vol, ptrs,
               [signed(seed & 0xffffffff), signed(seed >> 32), draw],
               [float(hubble)] if wkb else [])


# ---------------------------------------------------------------------------
# multigrid transfers (K15/K16): restriction and prolongation between a
# halo-padded fine array f1 (interior 2*n2 per axis) and a halo-padded
# coarse array f2 (interior n2), one launch each.  The per-axis
# coefficients and the halo are baked in as literals; the coarse extents
# and the number of outer slices are run-time ints, so one operator
# compiles once per dtype and serves every level.  Every loaded value is
# widened once to double, the tensor-product sum is evaluated in double
# one axis after the other (in the torch chain's order: x, y, z for
# restriction, z, y, x for prolongation), and each stored value is
# rounded once to ``real``; the ``correct`` forms store one rounding of
# ``(double)old - R(f1)`` and ``(double)old + I(f2)``.  Products may
# contract into multiply-adds: the result is defined to rounding, not to
# the bits of the torch chain in multigrid/transfer.py.
#
# A block is MG_TY waves; a wave is 64 consecutive sites of one z-row of
# the kernel's lane axis (coarse k for restriction, fine k for
# prolongation), the block's waves are MG_TY consecutive coarse j, and
# each thread walks MG_XI consecutive coarse i.  Rows and planes that
# neighbouring sites share are therefore re-read from L1/L2 by the same
# block shortly after their first read.  Tiles never straddle an outer
# slice; the grid is capped and strides over the tiles.  Only interior
# sites of the output are stored.

MG_TY = 4
MG_XI = 4
_MG_GRID_CAP = 4096

MG_TRANSFER_TEMPLATE = """#define H {halo}
#define TY {ty}
#define XI {xi}
using real = {real};

extern "C" __global__ __launch_bounds__(64 * TY) void {name}(
    {params},
    const int n2x, const int n2y, const int n2z, const int nouter)
{{
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    // strides of the fine (1) and coarse (2) padded arrays
    const long sy1 = 2L * n2z + 2 * H, sx1 = sy1 * (2L * n2y + 2 * H);
    const long so1 = sx1 * (2L * n2x + 2 * H);
    const long sy2 = (long)n2z + 2 * H, sx2 = sy2 * ((long)n2y + 2 * H);
    const long so2 = sx2 * ((long)n2x + 2 * H);
    const int nlz = {lane_extent};
    const int ntz = (nlz + 63) / 64, nty = (n2y + TY - 1) / TY;
    const int ntx = (n2x + XI - 1) / XI;
    const long ntiles = (long)nouter * ntx * nty * ntz;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {{
        const int tz = (int)(t % ntz);
        long q = t / ntz;
        const int ty = (int)(q % nty);
        q /= nty;
        const int tx = (int)(q % ntx);
        const long o = q / ntx;
        const int lz = tz * 64 + lane, j = ty * TY + row;
        if (lz >= nlz || j >= n2y) continue;
        const int i1 = (tx * XI + XI < n2x) ? tx * XI + XI : n2x;
        for (int i = tx * XI; i < i1; ++i) {{
            {body}
        }}
    }}
}}
"""


def _mg_literal(c):
    c = float(c)
    if not math.isfinite(c):
        raise ValueError(f"transfer coefficient {c} is not finite")
    return repr(c)


def _mg_offset(a, stride):
    """``+ a * stride`` as source text (nothing for ``a == 0``)."""
    if a == 0:
        return ""
    return f" {'+' if a > 0 else '-'} {abs(a)} * {stride}"


def _mg_sum(terms):
    """Source of ``Σ c * value`` over ``terms``, pairs of (coefficient,
    double-valued source text); ``0.0`` for none."""
    if not terms:
        return "0.0"
    return " + ".join(f"{_mg_literal(c)} * {v}" for c, v in terms)


def _mg_axis_offsets(coefs, halo, what):
    out = {}
    for a, c in coefs.items():
        if int(a) != a:
            raise ValueError(f"{what} offset {a!r} is not an integer")
        out[int(a)] = c
    if not out:
        raise ValueError(f"{what} coefficients are empty")
    if max(abs(a) for a in out) > halo:
        raise ValueError(
            f"{what} offsets {sorted(out)} do not fit halo {halo}")
    return dict(sorted(out.items()))


def mg_interpolation_offsets(even, odd):
    """The per-parity ``{coarse offset: coefficient}`` of a prolongation
    (fine site ``2i + p`` takes ``Σ_a c_a f2[i + (p + a) // 2]``): the
    rule of ``InterpolationBase._axis_coefs``."""
    return tuple({(p + a) // 2: c for a, c in coefs.items()}
                 for p, coefs in enumerate((even, odd)))


def _mg_restrict_body(coefs, correct):
    items = list(coefs.items())
    lines = ["const real* __restrict__ p = f1 + o * so1 "
             "+ (H + 2L * i) * sx1 + (H + 2L * j) * sy1 + (H + 2L * lz);"]
    for na, (a, _) in enumerate(items):
        for nb, (b, _) in enumerate(items):
            lines.append(
                f"const real* __restrict__ r{na}_{nb} = p"
                f"{_mg_offset(a, 'sx1')}{_mg_offset(b, 'sy1')};")
    # x, then y, then z, each in ascending offset: the torch chain's
    # order, so that float64 results with coefficients whose products
    # are exact (full weighting's) are the chain's, bit for bit
    for nc, (cc, _) in enumerate(items):
        for nb in range(len(items)):
            lines.append(f"const double x{nb}_{nc} = " + _mg_sum(
                [(c, f"(double)r{na}_{nb}[{cc}]")
                 for na, (_, c) in enumerate(items)]) + ";")
        lines.append(f"const double y{nc} = " + _mg_sum(
            [(c, f"x{nb}_{nc}") for nb, (_, c) in enumerate(items)]) + ";")
    lines.append("const double s = " + _mg_sum(
        [(c, f"y{nc}") for nc, (_, c) in enumerate(items)]) + ";")
    lines.append("const long d = o * so2 + (H + (long)i) * sx2 "
                 "+ (H + (long)j) * sy2 + (H + lz);")
    lines.append("f2[d] = (real)((double)f2[d] - s);" if correct
                 else "f2[d] = (real)s;")
    return lines


def _mg_interpolate_body(par, correct):
    # the union of both parities' coarse offsets: what the pair of fine
    # sites 2i, 2i+1 reads along one axis
    union = sorted(set(par[0]) | set(par[1]))
    lines = ["const int pk = lz & 1;",
             "const real* __restrict__ pc = f2 + o * so2 "
             "+ (H + (long)i) * sx2 + (H + (long)j) * sy2 "
             "+ (H + (lz >> 1));"]
    # z: the lane's parity selects each coefficient, 0.0 where its
    # parity does not read the site, and every lane loads the whole
    # union.  Selecting the sums instead lets the compiler sink the
    # loads of one parity under an exec-masked branch per load.  (A
    # non-finite coarse value therefore reaches both fine sites of its
    # pair, where the chain confines it to the parity that reads it.)
    for nc, cc in enumerate(union):
        lines.append(
            f"const double cz{nc} = pk ? {_mg_literal(par[1].get(cc, 0.0))}"
            f" : {_mg_literal(par[0].get(cc, 0.0))};")
    for na, a in enumerate(union):
        for nb, b in enumerate(union):
            lines.append(
                f"const real* __restrict__ r{na}_{nb} = pc"
                f"{_mg_offset(a, 'sx2')}{_mg_offset(b, 'sy2')};")
            lines.append(f"const double z{na}_{nb} = " + " + ".join(
                f"cz{nc} * (double)r{na}_{nb}[{cc}]"
                for nc, cc in enumerate(union)) + ";")
    # y then x: both parities of both axes are this thread's, unrolled
    for na, a in enumerate(union):
        for pj in (0, 1):
            lines.append(f"const double y{na}_{pj} = " + _mg_sum(
                [(par[pj][b], f"z{na}_{nb}")
                 for nb, b in enumerate(union) if b in par[pj]]) + ";")
    lines.append("const long d = o * so1 + (H + 2L * i) * sx1 "
                 "+ (H + 2L * j) * sy1 + (H + lz);")
    for pi in (0, 1):
        for pj in (0, 1):
            val = _mg_sum([(par[pi][a], f"y{na}_{pj}")
                           for na, a in enumerate(union) if a in par[pi]])
            at = "d" + (" + sx1" if pi else "") + (" + sy1" if pj else "")
            lines.append(f"const double s{pi}{pj} = {val};")
            lines.append(
                f"f1[{at}] = (real)((double)f1[{at}] + s{pi}{pj});"
                if correct else f"f1[{at}] = (real)s{pi}{pj};")
    return lines


def _mg_kernel_name(kind, correct):
    return f"mg_{kind}" + ("_correct" if correct else "")


def _mg_dtype(dtype):
    if isinstance(dtype, str):
        dtype = getattr(torch, dtype, None)
    if dtype not in _RTYPE:
        raise TypeError(
            f"multigrid transfers take float32 or float64, got {dtype}")
    return dtype


def mg_transfer_source(kind, coefs, halo, dtype, correct=False):
    """HIP source of a multigrid transfer kernel.  ``kind`` is
    ``"restrict"`` with ``coefs`` the per-axis ``{fine offset:
    coefficient}``, or ``"interpolate"`` with ``coefs`` the pair
    ``(even, odd)`` of per-axis ``{offset: coefficient}`` of the even
    and odd fine sites.  ``halo`` is the padding of both arrays and
    ``dtype`` their element type.  Needs no device."""
    halo = int(halo)
    correct = bool(correct)
    real = _RTYPE[_mg_dtype(dtype)]
    if kind == "restrict":
        body = _mg_restrict_body(
            _mg_axis_offsets(coefs, halo, "restriction"), correct)
        params = ["const real* __restrict__ f1", "real* __restrict__ f2"]
        lane_extent = "n2z"
    elif kind == "interpolate":
        even, odd = coefs
        par = tuple(_mg_axis_offsets(c, halo, "prolongation") for c in
                    mg_interpolation_offsets(even, odd))
        body = _mg_interpolate_body(par, correct)
        params = ["real* __restrict__ f1", "const real* __restrict__ f2"]
        lane_extent = "2 * n2z"
    else:
        raise ValueError(f"unknown transfer kind {kind!r}")
    return MG_TRANSFER_TEMPLATE.format(
        halo=halo, ty=MG_TY, xi=MG_XI, real=real,
        name=_mg_kernel_name(kind, correct), params=",\n    ".join(params),
        lane_extent=lane_extent, body="\n            ".join(body))


_mg_cache = {}


def mg_transfer_fits(f1, f2, halo):
    """Whether fine ``f1`` and coarse ``f2`` are a pair the transfer
    kernels take: contiguous device tensors on one device, both float32
    or both float64, equal outer dimensions, last three dimensions
    exactly ``2 n2 + 2 halo`` and ``n2 + 2 halo``, no shared memory."""
    if not (isinstance(f1, torch.Tensor) and isinstance(f2, torch.Tensor)
            and f1.is_cuda and f2.is_cuda and f1.device == f2.device
            and f1.dtype == f2.dtype and f1.dtype in _RTYPE
            and f1.dim() >= 3 and f1.dim() == f2.dim()
            and f1.shape[:-3] == f2.shape[:-3]
            and f1.is_contiguous() and f2.is_contiguous()):
        return False
    for s1, s2 in zip(f1.shape[-3:], f2.shape[-3:]):
        n2 = s2 - 2 * halo
        if n2 < 0 or s1 != 2 * n2 + 2 * halo:
            return False
    a, b = f1.data_ptr(), f2.data_ptr()
    return (a + f1.numel() * f1.element_size() <= b
            or b + f2.numel() * f2.element_size() <= a)


def _mg_launch(kind, f1, f2, coefs, key, halo, correct):
    halo = int(halo)
    correct = bool(correct)
    if not mg_transfer_fits(f1, f2, halo):
        raise ValueError(
            f"mg_{kind}: f1 {tuple(f1.shape)} {f1.dtype} and f2 "
            f"{tuple(f2.shape)} {f2.dtype} are not a contiguous, "
            f"non-overlapping fine/coarse pair at halo {halo}")
    kid = _cached_kernel(
        _mg_cache, (kind, key, halo, f1.dtype, correct),
        _mg_kernel_name(kind, correct),
        lambda: mg_transfer_source(kind, coefs, halo, f1.dtype, correct))
    n2 = [s - 2 * halo for s in f2.shape[-3:]]
    nouter = 1
    for s in f2.shape[:-3]:
        nouter *= s
    nlz = n2[2] if kind == "restrict" else 2 * n2[2]
    ntiles = (nouter * ((n2[0] + MG_XI - 1) // MG_XI)
              * ((n2[1] + MG_TY - 1) // MG_TY) * ((nlz + 63) // 64))
    if ntiles == 0:
        return
    ext().jit_launch(kid, min(_MG_GRID_CAP, ntiles), 1, 1, 64 * MG_TY, 1, 1,
                     0, _stream(), [f1.data_ptr(), f2.data_ptr()],
                     n2 + [nouter], [])


def _mg_key(coefs):
    return tuple(sorted((int(a), float(c)) for a, c in coefs.items()))


def mg_restrict(f1, f2, coefs, halo, correct):
    """One launch, no allocation: the interior of coarse ``f2`` becomes
    (``correct``: is reduced by) ``Σ_abc c_a c_b c_c f1[2i+a, 2j+b,
    2k+c]`` of fine ``f1``.  Returns without a launch if the coarse
    interior is empty."""
    _mg_launch("restrict", f1, f2, coefs, _mg_key(coefs), halo, correct)


def mg_interpolate(f1, f2, even, odd, halo, correct):
    """One launch, no allocation: the interior of fine ``f1`` becomes
    (``correct``: is increased by) the tensor-product prolongation of
    coarse ``f2`` with per-axis coefficients ``even`` and ``odd``."""
    _mg_launch("interpolate", f1, f2, (even, odd),
               (_mg_key(even), _mg_key(odd)), halo, correct)


# ---------------------------------------------------------------------------
# AOT stencil kernels (csrc/derivs.hip)

def _flat_fields(t, ndim_grid=3):
    """Collapse outer axes; returns (tensor_view, nf)."""
    outer = t.shape[:-ndim_grid]
    nf = int(np.prod(outer)) if outer else 1
    return t, nf


_DERIV_DTYPES = {torch.float64: 0, torch.float32: 1}


def _deriv_dtype(name, t):
    code = _DERIV_DTYPES.get(t.dtype)
    if code is None:
        raise TypeError(f"{name}: stencil kernels support fp64/fp32, "
                        f"got {t.dtype}")
    return code


def derivs(fx, lap=None, pdx=None, pdy=None, pdz=None, grd=None, halo=None,
           dx=None, h=None, stream=True):
    if len(set(halo)) != 1:
        raise NotImplementedError("GPU stencils require isotropic halo")
    _check_tensor("fx", fx)
    dtype = _deriv_dtype("fx", fx)
    esize = fx.element_size()
    nxp, nyp, nzp = fx.shape[-3:]
    nx, ny, nz = nxp - 2 * h, nyp - 2 * h, nzp - 2 * h
    _, nf = _flat_fields(fx)
    uvol = nx * ny * nz

    def ptr(t):
        if t is None:
            return 0
        _check_tensor("out", t)
        if t.dtype != fx.dtype:
            raise TypeError(f"output dtype {t.dtype} != input {fx.dtype}")
        return t.data_ptr()

    e = ext()
    # gradient outputs: either a packed (..., 3, nx, ny, nz) grd array
    # (per-field component stride 3*uvol) or three standalone arrays
    if grd is not None and isinstance(grd, torch.Tensor):
        _check_tensor("grd", grd)
        gp = ptr(grd)
        px, py, pz_ = gp, gp + esize * uvol, gp + 2 * esize * uvol
        g_fstride = 3 * uvol
        want_grad = True
    elif pdx is not None and pdy is not None and pdz is not None:
        px, py, pz_ = ptr(pdx), ptr(pdy), ptr(pdz)
        g_fstride = uvol
        want_grad = True
    else:
        px = py = pz_ = 0
        g_fstride = 0
        want_grad = False

    if lap is not None or want_grad:
        e.gradlap(fx.data_ptr(), ptr(lap), px, py, pz_, g_fstride,
                  h, nx, ny, nz, nf, dx[0], dx[1], dx[2], dtype,
                  _stream())
        return
    # single-axis derivatives
    for axis, out in enumerate((pdx, pdy, pdz)):
        if out is not None:
            e.pd(fx.data_ptr(), ptr(out), h, axis, 0, nx, ny, nz, nf,
                 dx[axis], dtype, _stream())


def divergence(vec, div, halo=None, dx=None, h=None):
    _check_tensor("vec", vec)
    _check_tensor("div", div)
    dtype = _deriv_dtype("vec", vec)
    if div.dtype != vec.dtype:
        raise TypeError(f"div dtype {div.dtype} != vec {vec.dtype}")
    nxp, nyp, nzp = vec.shape[-3:]
    nx, ny, nz = nxp - 2 * h, nyp - 2 * h, nzp - 2 * h
    outer = vec.shape[:-4]
    e = ext()
    from itertools import product
    for s in product(*[range(n) for n in outer]):
        e.pd(vec[s][0].data_ptr(), div[s].data_ptr(), h, 0, 0,
             nx, ny, nz, 1, dx[0], dtype, _stream())
        e.pd(vec[s][1].data_ptr(), div[s].data_ptr(), h, 1, 1,
             nx, ny, nz, 1, dx[1], dtype, _stream())
        e.pd(vec[s][2].data_ptr(), div[s].data_ptr(), h, 2, 1,
             nx, ny, nz, 1, dx[2], dtype, _stream())


# ---------------------------------------------------------------------------
# Fused Laplacian + reduction kernel (MI355X-specific optimization).
#
# The reference hot loop runs the stencil pass and the energy reduction
# as separate kernels (reference examples/scalar_preheating.py:258-271 →
# derivs.py:339-429 then reduction.py:206); that re-reads f and lap_f
# from HBM.  Here one x-marching pass computes lap (register ring +
# current-plane neighbor loads), stores it, and accumulates the energy
# reductions with the freshly computed Laplacian still in registers:
# HBM traffic per site drops from (f, lap w, f, dfdt, lap r) to
# (f, dfdt, lap w).

def _real_name(dtype):
    """C name of the per-site type in the generated ring kernels.  The
    float64 kernels spell it ``double`` (their source text is pinned:
    the tuned flagship kernels must not move), every other dtype uses
    the ``real`` alias that ``geometry_defines`` sets."""
    if dtype not in _RTYPE:
        raise TypeError(f"unsupported kernel dtype {dtype}")
    return "double" if dtype == torch.float64 else "real"


def _lapc0_define(lapc0, dtype):
    if dtype == torch.float64:
        return f"#define LAPC0 ({lapc0!r})\n"
    return f"#define LAPC0 (real({lapc0!r}))\n"


def _lap_stencil_pieces(h, dx, periodic, dtype=torch.float64):
    """Shared codegen for the inline-Laplacian ring kernels: stencil
    term strings, the center coefficient, the x-ring load/init forms
    and the accumulator's initialization.  periodic=(px,py,pz) wraps
    that axis's stencil reads in-kernel (star stencil) so
    non-decomposed axes need NO halo fill.

    float64 evaluates ``c0*f0 + sum_s c_s (f[+s] + f[-s])``.  Below
    float64 the coefficients (16/12, 1/12, ...) are inexact, no longer
    sum to zero, and the field's mean leaks into the Laplacian (1.3e-6
    absolute at h=2 for the 0.193 inflaton mean, more than a 1e-6
    fluctuation's whole signal), so those kernels use the difference
    form ``sum_s c_s ((f[+s] - f0) + (f[-s] - f0))``: the mean cancels
    exactly before any coefficient is applied, at two subtractions per
    neighbour pair in a bandwidth-bound kernel.
    """
    from pystella_amd.derivs import _LAP_COEFS
    inv2 = [1.0 / d / d for d in dx]
    coefs = _LAP_COEFS[h]
    px_, py_, pz_ = periodic
    wrap_decls = []
    lap_terms = []
    for s in range(1, h + 1):
        c = coefs[s]
        if py_:
            wrap_decls.append(
                f"const long ypo{s} = ((j + {s} < NY) ? {s}L "
                f": {s}L - NY) * PSZ;")
            wrap_decls.append(
                f"const long ymo{s} = ((j >= {s}) ? -{s}L "
                f": NY - {s}L) * PSZ;")
            yp, ym = f"ypo{s}", f"ymo{s}"
        else:
            yp, ym = f"{s}*PSZ", f"-{s}*PSZ"
        if pz_:
            wrap_decls.append(
                f"const int zpo{s} = (k + {s} < NZ) ? {s} "
                f": {s} - NZ;")
            wrap_decls.append(
                f"const int zmo{s} = (k >= {s}) ? -{s} "
                f": NZ - {s};")
            zp, zm = f"zpo{s}", f"zmo{s}"
        else:
            zp, zm = f"{s}", f"-{s}"
        if dtype == torch.float64:
            lap_terms.append(
                f"la += {c!r} * ((ring[fld][H+{s}] + ring[fld][H-{s}])"
                f"*{inv2[0]!r} + (cp[{yp}] + cp[{ym}])*{inv2[1]!r}"
                f" + (cp[{zp}] + cp[{zm}])*{inv2[2]!r});")
        else:
            lap_terms.append(
                f"la += real({c!r}) * ("
                f"((ring[fld][H+{s}] - f0) + (ring[fld][H-{s}] - f0))"
                f"*real({inv2[0]!r})"
                f" + ((cp[{yp}] - f0) + (cp[{ym}] - f0))"
                f"*real({inv2[1]!r})"
                f" + ((cp[{zp}] - f0) + (cp[{zm}] - f0))"
                f"*real({inv2[2]!r}));")
    lapc0 = coefs[0] * (inv2[0] + inv2[1] + inv2[2])
    if dtype == torch.float64:
        la_init = "double la = ring[fld][H] * LAPC0;"
    else:
        la_init = "const real f0 = ring[fld][H]; real la = real(0.0);"
    if px_:
        x_off = ("int xq = i + 2 * H; "
                 "if (xq >= NX + H) xq -= NX;")
        ring_load = "ring[fld][2 * H] = fp[(long)xq * sx];"
        ring_init = ("int xq0 = i0 + p; "
                     "if (xq0 < H) xq0 += NX; "
                     "if (xq0 >= NX + H) xq0 -= NX; "
                     "ring[fld][p] = fp[(long)xq0 * sx];")
    else:
        x_off = ""
        ring_load = "ring[fld][2 * H] = fp[(long)(i + 2 * H) * sx];"
        ring_init = "ring[fld][p] = fp[(long)(i0 + p) * sx];"
    return (wrap_decls, lap_terms, lapc0, x_off, ring_load, ring_init,
            la_init)



# The x-march of every ring kernel, written once: ring fill, then per
# site the ring load, the per-field Laplacian (stored if the form says
# so), ``{body}`` and the ring shift, then the partials tail.  A form
# (_FORM_GRID, _FORM_BOX, _FORM_SHELL) says where a block finds its
# sites (``{prologue}`` yields k, j, i0 and i1; ``{kmax}``/``{jmax}``
# bound k and j; ``{tables}`` precedes the kernel) and which column of
# the partials buffer is its own (``{bid}``, ``{stride}``); _ring_source
# fills it in.
RING_MARCH_TEMPLATE = """{defines}
{preamble}
#define NRED {nred}
#define NF {nf}
{tables}extern "C" __global__ __launch_bounds__({bounds}) void {name}(
    {params})
{{
    double acc[NRED];
    {init}
    {prologue}
    if (k < {kmax} && j < {jmax}) {{
        const long sx = PSY * PSZ;
        {wrap_decls}
        {outer_decls}
        #pragma unroll
        for (int fld = 0; fld < NF; ++fld) {{
            const {R}* fp = {fname} + (long)fld * PVOL
                               + (long)(j + H) * PSZ + (k + H);
            #pragma unroll
            for (int p = 0; p < 2 * H; ++p) {{
                {ring_init}
            }}
        }}
        for (int i = i0; i < i1; ++i) {{
            {site_decls}
            {x_off}
            #pragma unroll
            for (int fld = 0; fld < NF; ++fld) {{
                const {R}* fp = {fname} + (long)fld * PVOL
                                   + (long)(j + H) * PSZ + (k + H);
                {ring_load}
                const {R}* cp = fp + (long)(i + H) * sx;
                {la_init}
                {lap_terms}
                lapv[fld] = la;{store_lap}
            }}
            {body}
            #pragma unroll
            for (int fld = 0; fld < NF; ++fld)
                #pragma unroll
                for (int p = 0; p < 2 * H; ++p)
                    ring[fld][p] = ring[fld][p + 1];
        }}
    }}
""" + PARTIALS_TAIL

# ``{store_lap}`` of the kernels that can keep the Laplacian
_STORE_LAP = """
#if STORE_LAP
                {lapname}[(long)fld * UVOL + (((long)i * NY + j) * NZ + k)]
                    = la;
#endif"""

# the whole grid, one launch with a partials buffer of its own
_FORM_GRID = dict(
    tables="",
    prologue="""const int k = blockIdx.x * TBZ + (threadIdx.x % TBZ);
    const int j = blockIdx.y * TBY + (threadIdx.x / TBZ);
    const int i0 = blockIdx.z * XCHUNK;
    const int i1 = (i0 + XCHUNK < NX) ? i0 + XCHUNK : NX;""",
    kmax="NZ", jmax="NY", bid=_GRID_BID, stride="nblk")

# a box passed as ints; sub-box launches of the same kernel write
# disjoint slices (from column bid0) of one shared partials buffer
_FORM_BOX = dict(
    tables="",
    prologue="""const int k = k0b + blockIdx.x * TBZ + (threadIdx.x % TBZ);
    const int j = j0b + blockIdx.y * TBY + (threadIdx.x / TBZ);
    const int i0 = i0b + blockIdx.z * XCHUNK;
    const int i1 = (i0 + XCHUNK < i1b) ? i0 + XCHUNK : i1b;""",
    kmax="k1b", jmax="j1b",
    bid="""const int bid = bid0 + (blockIdx.z * gridDim.y + blockIdx.y)
                    * gridDim.x + blockIdx.x;""",
    stride="nblkT")

# Multi-box "shell" form: ONE launch covers all boundary slabs of a
# rank (separate thin-slab launches are latency-bound at ~1 wave/CU
# each and serialize).  Box bounds and per-box block-grid tables are
# baked as constant arrays; blocks decode their (box, tile) from the
# flat blockIdx.x, and the reduction tail indexes partials by the flat
# block id.
_SHELL_TABLES = """#define NBOX {nbox}
__constant__ int sh_k0[NBOX] = {{ {k0s} }};
__constant__ int sh_k1[NBOX] = {{ {k1s} }};
__constant__ int sh_j0[NBOX] = {{ {j0s} }};
__constant__ int sh_j1[NBOX] = {{ {j1s} }};
__constant__ int sh_i0[NBOX] = {{ {i0s} }};
__constant__ int sh_i1[NBOX] = {{ {i1s} }};
__constant__ int sh_gz[NBOX] = {{ {gzs} }};
__constant__ int sh_gy[NBOX] = {{ {gys} }};
__constant__ int sh_blk0[NBOX] = {{ {blk0s} }};
"""

_FORM_SHELL = dict(
    prologue="""const int bflat = (int)blockIdx.x;
    int box = 0;
    #pragma unroll
    for (int b = 1; b < NBOX; ++b) box += (bflat >= sh_blk0[b]);
    const int lb = bflat - sh_blk0[box];
    const int bz = lb % sh_gz[box];
    const int by = (lb / sh_gz[box]) % sh_gy[box];
    const int bx = lb / (sh_gz[box] * sh_gy[box]);
    const int k = sh_k0[box] + bz * TBZ + (int)(threadIdx.x % TBZ);
    const int j = sh_j0[box] + by * TBY + (int)(threadIdx.x / TBZ);
    const int i0 = sh_i0[box] + bx * XCHUNK;
    const int i1 = (i0 + XCHUNK < sh_i1[box]) ? i0 + XCHUNK
                                              : sh_i1[box];""",
    kmax="sh_k1[box]", jmax="sh_j1[box]",
    bid="const int bid = bid0 + bflat;", stride="nblkT")


def _ring_source(parts, form, **over):
    """RING_MARCH_TEMPLATE filled with a kernel's ``parts`` for
    ``form``.  Where ``lapv[]`` is declared goes with the form: the
    shell form has it outside the x-loop, the others inside, and the
    compiler's register allocation follows the place (the GW shell
    kernels at MINW 2 come out different if it moves)."""
    lapv = "{R} lapv[NF];".format(**parts)
    ring = "{R} ring[NF][2 * H + 1];".format(**parts)
    if form is _FORM_SHELL:
        decls = dict(outer_decls=f"{lapv}\n        {ring}", site_decls="")
    else:
        decls = dict(outer_decls=ring, site_decls=lapv)
    return RING_MARCH_TEMPLATE.format(
        **{**parts, **form, **decls, **over})


def _march_pieces(f_name, halo, dx, periodic, dtype):
    """(RING_MARCH_TEMPLATE's stencil fields, the LAPC0 define) for the
    stencil field ``f_name``."""
    h = max(halo) if isinstance(halo, (tuple, list)) else halo
    (wrap_decls, lap_terms, lapc0, x_off, ring_load, ring_init,
     la_init) = _lap_stencil_pieces(h, dx, periodic, dtype)
    return dict(
        R=_real_name(dtype), fname=f_name,
        wrap_decls="\n        ".join(wrap_decls), x_off=x_off,
        ring_load=ring_load, ring_init=ring_init, la_init=la_init,
        lap_terms="\n                ".join(lap_terms),
    ), _lapc0_define(lapc0, dtype)


class _RingKernel(_PartialsKernel):
    """Host side of the register-ring Laplacian kernels."""

    state_map = None

    def _declare_ring(self, cg, field_args, f_name, lap_name, R,
                      store_lap=False, ints=()):
        """The parameter list of a ring kernel: stencil field first, the
        Laplacian if stored, the other spatial fields sorted, the
        device-state buffer if any, partials, ints, then the run-time
        scalars ``cg`` collected so far."""
        names = [f_name] + ([lap_name] if store_lap else []) + sorted(
            fa.name for fa in field_args
            if fa.spatial and fa.name not in (f_name, lap_name))
        by_name = {fa.name: fa for fa in field_args}
        self.field_args = [by_name[n] for n in names if n in by_name]
        if self.state_map:
            names.append("state")
        return self._declare(
            cg, names,
            lambda n: ("const double* __restrict__ state" if n == "state"
                       else f"{R}* __restrict__ {n}"),
            [self.PARTIALS] + list(ints))

    def _arg_dtype(self, name):
        # the device-state scalar buffer is float64 whatever the fields are
        return torch.float64 if name == "state" and self.state_map \
            else self.dtype


class _LapCodegen(Codegen):
    """Codegen that maps accesses to the stencil field's center value and
    the freshly computed Laplacian onto kernel registers."""

    def __init__(self, field_args, halo, rank_shape, f_name, lap_name):
        super().__init__(field_args, halo, rank_shape)
        self.f_name = f_name
        self.lap_name = lap_name
        # set while a reducer's per-site value is emitted in a kernel
        # whose real is narrower than double: run-time scalars enter
        # there as the doubles they are passed as.  Narrowed, the scale
        # factor would be off by up to 6e-8, the same at every site, so
        # the kinetic and gradient energies that feed the float64
        # Friedmann ODE would carry twice that instead of averaging
        # their rounding away.  The field part of the value is still
        # evaluated in real and widens where the scalar meets it.
        self.wide_scalars = False

    def scalar_param(self, name, idx=()):
        v = super().scalar_param(name, idx)
        if self.wide_scalars and v.startswith("real(s_"):
            return v[len("real("):-1]
        return v

    def field_access(self, f, outer_idx):
        if f.is_spatial and not any(f.shift) and len(outer_idx) <= 1:
            lin = int(outer_idx[0]) if outer_idx else 0
            if f.name == self.lap_name:
                return f"lapv[{lin}]"
            if f.name == self.f_name:
                return f"ring[{lin}][H]"
        return super().field_access(f, outer_idx)


class JitLapReduction(_RingKernel):
    """Fused lap-stencil + multi-quantity reduction (see module note)."""

    def __init__(self, entries, field_args, scalar_names, halo, rank_shape,
                 dx, nf, f_name="f", lap_name="lap_f", name="lapred_map",
                 tile=(64, 4, 64), store_lap=True, dtype=torch.float64,
                 compile=True):
        self.rank_shape = tuple(rank_shape)
        self.tile = tile
        self.dtype = dtype
        self.store_lap = store_lap
        self.entries = entries
        self.nf = nf
        # the stencil reads the halo on every axis
        self.periodic = (False, False, False)
        march, lapc0 = _march_pieces(f_name, halo, dx, self.periodic, dtype)
        R = march["R"]
        cg = _LapCodegen(field_args, halo, rank_shape, f_name, lap_name)
        if R == "real":
            cg.one = "real(1.0)"
        init_lines, body_lines, combine = _reducer_pieces(
            cg, entries, wide_scalars=R == "real")
        params = self._declare_ring(cg, field_args, f_name, lap_name, R,
                                    store_lap=store_lap)

        defines = geometry_defines(halo, rank_shape, rtype=_RTYPE[dtype])
        defines += _tile_defines(tile)
        defines += combine + lapc0
        defines += f"#define STORE_LAP {1 if store_lap else 0}\n"
        self._build(_ring_source(dict(
            defines=defines, preamble=PREAMBLE, nred=len(entries), nf=nf,
            bounds="TBZ * TBY", name=name, params=params,
            init="\n    ".join(init_lines),
            store_lap=_STORE_LAP.format(lapname=lap_name),
            body="\n            ".join(body_lines), **march), _FORM_GRID),
            name, compile)
        self._tiled(tile, rank_shape)


class _NTLapCodegen(_LapCodegen):
    """_LapCodegen plus read-redirection to nontemporal preloads and
    device-state scalars (scalars read from a device buffer instead of
    being passed by value — lets the whole RK step run without host
    synchronization, see JitFriedmann)."""

    def __init__(self, *args, state_map=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.preload = {}       # (name, lin) -> register var
        self.store_ctx = False
        self.state_map = state_map or {}

    def scalar_param(self, name, idx=()):
        # state scalars are hoisted into per-thread registers once at
        # kernel entry (st_<name>, see _state_prologue)
        if name in self.state_map and not idx:
            return f"std_{name}" if self.wide_scalars else f"st_{name}"
        return super().scalar_param(name, idx)

    def field_access(self, f, outer_idx):
        if (not self.store_ctx and f.is_spatial
                and len(outer_idx) <= 1 and not any(f.shift)):
            lin = int(outer_idx[0]) if outer_idx else 0
            reg = self.preload.get((f.name, lin))
            if reg is not None:
                return reg
        return super().field_access(f, outer_idx)


def _nt_preloads(field_args, lap_name, exprs):
    """Sorted (name, component) of every component of the unpadded
    streaming arrays (the RK k-arrays) that ``exprs`` read: each is
    preloaded once per site with a nontemporal load."""
    from pystella_amd.field import Field, Subscript, iter_exprs, walk_expr
    nt_names = {fa.name for fa in field_args
                if fa.spatial and not fa.padded and fa.name != lap_name
                and len(fa.outer_shape) <= 1}
    used = set()

    def visit(x):
        if isinstance(x, Subscript) and isinstance(x.aggregate, Field) \
                and x.aggregate.name in nt_names and len(x.index) == 1 \
                and isinstance(x.index[0], int):
            used.add((x.aggregate.name, int(x.index[0])))
        elif isinstance(x, Field) and x.name in nt_names and not x.shape:
            used.add((x.name, 0))

    for e in iter_exprs(exprs):
        walk_expr(e, visit)
    return sorted(used)


def _preload_decl(R, nm, lin):
    off = "(((long)i*NY + j)*NZ + k)"
    if lin:
        off = f"({lin}L*UVOL + {off})"
    return (f"const {R} pl_{nm}_{lin} = "
            f"__builtin_nontemporal_load(&{nm}[{off}]);")


def _store_lines(cg, items, nt):
    lines = []
    for lhs, rhs in items:
        val = cg.emit(rhs)
        cg.store_ctx = True
        dst = cg.emit(lhs)
        cg.store_ctx = False
        if nt:
            lines.append(f"__builtin_nontemporal_store({val}, &{dst});")
        else:
            lines.append(f"{dst} = {val};")
    return lines


def _stage_site_body(cg, R, tmp_items, entries, store_items, preloads,
                     nt):
    """(site lines, ``acc[]`` init lines, COMBINE define) of a stage
    kernel.  Per site: k-array preloads, temporaries, the reducers
    (so they see the input state), then the stores."""
    for lhs, _ in tmp_items:
        cg.tmp_names.add(lhs.name if hasattr(lhs, "name") else str(lhs))
    lines = []
    for nm, lin in preloads:
        cg.preload[(nm, lin)] = f"pl_{nm}_{lin}"
        lines.append(_preload_decl(R, nm, lin))
    for lhs, rhs in tmp_items:
        tname = lhs.name if hasattr(lhs, "name") else str(lhs)
        lines.append(f"const {R} {tname} = {cg.emit(rhs)};")
    acc_init, acc_lines, combine = _reducer_pieces(
        cg, entries, wide_scalars=R == "real")
    lines += acc_lines
    lines += _store_lines(cg, store_items, nt)
    return lines, acc_init, combine


def _state_prologue(state_map, R):
    """Kernel-entry reads of the device-state scalars into registers."""
    lines = []
    for nm, sidx in sorted((state_map or {}).items()):
        if R == "double":
            lines.append(f"const double st_{nm} = state[{sidx}];")
        else:
            # narrowed once at kernel entry, so the per-site
            # expressions that use it stay in real; the reducers
            # take the double (see _LapCodegen.wide_scalars)
            lines.append(f"const double std_{nm} = state[{sidx}];")
            lines.append(f"const real st_{nm} = real(std_{nm});")
    return lines


class JitLapStage(_RingKernel):
    """Ring-buffer RK stage kernel fused with input-state reductions:
    the stencil field marches along x through a per-thread register ring
    (one new load per site instead of 4h+1), the Laplacian is formed in
    registers, the reducers accumulate input-state values, and the
    2N-storage update stores last.  The k-arrays are read once via
    nontemporal loads and every store is nontemporal (streaming data
    never pollutes the L2, which stays available for stencil-neighbor
    reuse).  This is the hot loop's only kernel
    (see fusion.StencilRKStepper).

    For large stencil families (the 6-component GW h_ij sector), the
    per-site emission keeps all 6 Laplacians + 12 k-preloads + ring
    live simultaneously — 256 VGPRs, 2 waves/SIMD, ~4.2 TB/s
    (measured round 1)."""

    # tile candidates, best-first for large grids; smaller tiles win on
    # small per-rank grids (multi-GPU strong scaling) where the big
    # tile cannot fill 256 CUs with enough workgroups
    TILE_CANDIDATES = ((64, 8, 64), (64, 4, 32), (64, 2, 16),
                       (32, 2, 8))

    @classmethod
    def pick_tile(cls, rank_shape):
        env = os.environ.get("PYSTELLA_TILE")
        if env:
            try:
                tile = tuple(int(x) for x in env.split(","))
            except ValueError:
                tile = ()
            if len(tile) != 3 or any(t <= 0 for t in tile):
                raise ValueError(
                    f"PYSTELLA_TILE={env!r}: expected three positive "
                    "integers 'TBZ,TBY,XCHUNK'")
            if (tile[0] * tile[1]) % 64:
                raise ValueError(
                    f"PYSTELLA_TILE={env!r}: block of TBZ*TBY = "
                    f"{tile[0] * tile[1]} threads is not a multiple of "
                    "the 64-lane wavefront")
            nthr = tile[0] * tile[1]
            if nthr & (nthr - 1) or nthr > 1024:
                # the LDS reduction tree halves the block each level
                raise ValueError(
                    f"PYSTELLA_TILE={env!r}: block of TBZ*TBY = {nthr} "
                    "threads must be a power of two, at most 1024")
            return tile
        for tile in cls.TILE_CANDIDATES:
            g = _tile_grid(tile, rank_shape)
            if g[0] * g[1] * g[2] >= 2048:
                return tile
        return max(cls.TILE_CANDIDATES,
                   key=lambda t: int(np.prod(_tile_grid(t, rank_shape))))

    def __init__(self, map_dict, tmp_instructions, entries, field_args,
                 scalar_names, halo, rank_shape, dx, nf, f_name="f",
                 lap_name="lap_f", name="rk_lapstage", tile=None,
                 nt=True, state_map=None, min_waves=1,
                 periodic=(False, False, False),
                 dtype=torch.float64, compile=True):
        if tile is None:
            tile = self.pick_tile(rank_shape)
        self.rank_shape = tuple(rank_shape)
        # dynamic-LDS ballast at launch: caps waves/CU without kernel
        # changes (occupancy throttling for cache-thrash regimes)
        self.shmem = 0
        self.tile = tile
        self.dtype = dtype
        self.entries = entries
        self.nf = nf
        self.state_map = state_map
        self.periodic = tuple(periodic)
        # per-site type R: arrays, ring, Laplacian, RHS and the 2N update;
        # acc[], the LDS tree, partials and the state buffer stay double
        march, lapc0 = _march_pieces(f_name, halo, dx, periodic, dtype)
        R = march["R"]
        cg = _NTLapCodegen(field_args, halo, rank_shape, f_name, lap_name,
                           state_map=state_map)
        if R == "real":
            cg.one = "real(1.0)"

        tmp_items = list((tmp_instructions or {}).items())
        preloads = _nt_preloads(
            field_args, lap_name,
            [[r for _, r in tmp_items], [e for e, _ in entries]]) \
            if nt else []
        lines, acc_init, combine = _stage_site_body(
            cg, R, tmp_items, entries, list(map_dict.items()), preloads,
            nt)
        params = self._declare_ring(
            cg, field_args, f_name, lap_name, R,
            ints=["const int k0b, const int k1b, const int j0b, "
                  "const int j1b, const int i0b, const int i1b, "
                  "const int nblkT, const int bid0"])

        defines = geometry_defines(halo, rank_shape, rtype=_RTYPE[dtype])
        defines += _tile_defines(tile)
        defines += f"#define MINW {min_waves}\n"
        defines += combine + lapc0
        # everything but the form: the shell form is rendered per set
        # of boxes (_shell_build)
        self._parts = dict(
            defines=defines, preamble=PREAMBLE, nred=len(entries), nf=nf,
            bounds="TBZ * TBY, MINW", name=name, params=params,
            init="\n    ".join(_state_prologue(state_map, R) + acc_init),
            store_lap="", body="\n            ".join(lines), **march)
        self._shell_cache = {}
        # compile=False leaves ``.source`` and ``shell_source``
        self._build(_ring_source(self._parts, _FORM_BOX), name, compile)
        self._tiled(tile, rank_shape)

    def _box_geometry(self, box):
        """(grid, ints-prefix) for a sub-box launch; box =
        (i0, i1, j0, j1, k0, k1) in interior coordinates."""
        tbz, tby, xchunk = self.tile
        i0, i1, j0, j1, k0, k1 = box
        grid = ((k1 - k0 + tbz - 1) // tbz,
                (j1 - j0 + tby - 1) // tby,
                (i1 - i0 + xchunk - 1) // xchunk)
        return grid, [k0, k1, j0, j1, i0, i1]

    def box_nblk(self, box):
        grid, _ = self._box_geometry(box)
        return grid[0] * grid[1] * grid[2]

    # -- multi-box shell launch (all boundary slabs in ONE kernel) ------
    def shell_source(self, boxes):
        """HIP source of the shell form over ``boxes`` (no device)."""
        return self._shell_build(tuple(boxes))[0]

    def _get_shell(self, boxes):
        cached = self._shell_cache.get(boxes)
        if cached is not None:
            return cached
        self._require_compiled()
        src, name, total = self._shell_build(boxes)
        cached = (ext().jit_compile(src, name), total)
        self._shell_cache[boxes] = cached
        return cached

    def _shell_build(self, boxes):
        grids = [self._box_geometry(b)[0] for b in boxes]
        nbs = [g[0] * g[1] * g[2] for g in grids]
        blk0 = [0]
        for n in nbs[:-1]:
            blk0.append(blk0[-1] + n)

        def ints(vals):
            return ", ".join(str(int(v)) for v in vals)

        tables = _SHELL_TABLES.format(
            nbox=len(boxes),
            k0s=ints(b[4] for b in boxes), k1s=ints(b[5] for b in boxes),
            j0s=ints(b[2] for b in boxes), j1s=ints(b[3] for b in boxes),
            i0s=ints(b[0] for b in boxes), i1s=ints(b[1] for b in boxes),
            gzs=ints(g[0] for g in grids), gys=ints(g[1] for g in grids),
            blk0s=ints(blk0))
        name = self._parts["name"] + "_shell"
        src = _ring_source(self._parts, _FORM_SHELL, name=name,
                           tables=tables)
        return src, name, sum(nbs)

    def shell_nblk(self, boxes):
        return self._get_shell(tuple(boxes))[1]

    def launch_shell(self, env, boxes, partials, bid0, nblk_tot):
        """ONE launch covering every box in ``boxes`` (the rank's
        boundary slabs); per-block partials land flat at ``bid0``."""
        ptrs, _ = self._pointers(env)
        kid, total = self._get_shell(tuple(boxes))
        self._launch(kid, (total, 1, 1), env, ptrs + [partials.data_ptr()],
                     [0, 0, 0, 0, 0, 0, nblk_tot, bid0])

    def launch_box(self, env, box, partials, bid0, nblk_tot):
        """Launch over a sub-box, writing this launch's per-block
        partials at column offset ``bid0`` of the shared ``partials``
        buffer [nred, nblk_tot].  Stream-ordered, no host sync."""
        ptrs, _ = self._pointers(env)
        grid, ints = self._box_geometry(box)
        self._launch(self.key, grid, env, ptrs + [partials.data_ptr()],
                     ints + [nblk_tot, bid0])

    def launch_only(self, env):
        nx, ny, nz = self.rank_shape
        return super().launch_only(
            env, [0, nz, 0, ny, 0, nx, self.nblk, 0])


FRIEDMANN_TEMPLATE = """
#define NRED {nred}
#define NBLK {nblk}
extern "C" __global__ __launch_bounds__(256) void {name}_sums(
    const double* __restrict__ partials, double* __restrict__ sums)
{{
    __shared__ double sd[256];
    const int r = blockIdx.x;
    double acc = 0.0;
    for (int c = threadIdx.x; c < NBLK; c += 256)
        acc += partials[(long)r * NBLK + c];
    sd[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {{
        if ((int)threadIdx.x < s)
            sd[threadIdx.x] += sd[threadIdx.x + s];
        __syncthreads();
    }}
    if (threadIdx.x == 0) sums[r] = sd[0];
}}

extern "C" __global__ void {name}_step(
    const double* __restrict__ sums, double* __restrict__ state,
    double A, double B, double dt)
{{
    const double wt[NRED] = {{ {wt} }};
    const double wp[NRED] = {{ {wp} }};
    double E = 0.0, P = 0.0;
    #pragma unroll
    for (int r = 0; r < NRED; ++r) {{
        const double avg = sums[r] * {inv_grid!r};
        E += wt[r] * avg;
        P += wp[r] * avg;
    }}
    const double a = state[0];
    const double adot = state[1];
    const double rhs_a = adot;
    const double rhs_adot = {frw_coef!r} * a * a * (E - 3.0 * P) * a;
    const double ka = A * state[2] + dt * rhs_a;
    const double kd = A * state[3] + dt * rhs_adot;
    const double an = a + B * ka;
    const double adn = adot + B * kd;
    state[0] = an;
    state[1] = adn;
    state[2] = ka;
    state[3] = kd;
    state[4] = adn / an;
    state[5] = E;
    state[6] = P;
}}
"""


class JitFriedmann:
    """Device-resident Friedmann update: finishes the stage kernel's
    per-block energy partials into E and P and advances the 2N-storage
    (a, adot) ODE — all on the stream, no host round trip.  The state
    buffer layout is [a, adot, k_a, k_adot, hubble, energy, pressure]
    (the stage kernels read a and hubble straight from it).

    Host analogue: :class:`pystella_amd.Expansion` (which mirrors
    reference pystella/expansion.py:28-176)."""

    STATE_A, STATE_ADOT, STATE_HUBBLE = 0, 1, 4
    STATE_ENERGY, STATE_PRESSURE = 5, 6

    def __init__(self, nred, nblk, wt, wp, grid_size, mpl=1.,
                 name="friedmann"):
        self.nred = nred
        self.nblk = nblk
        frw_coef = 4 * math.pi / 3 / mpl**2
        src = FRIEDMANN_TEMPLATE.format(
            nred=nred, nblk=nblk, name=name,
            wt=", ".join(repr(float(w)) for w in wt),
            wp=", ".join(repr(float(w)) for w in wp),
            inv_grid=1.0 / grid_size, frw_coef=frw_coef)
        self.source = src
        self.key_sums = ext().jit_compile(src, name + "_sums")
        self.key_step = ext().jit_compile(src, name + "_step")

    def finish_sums(self, partials, sums):
        ext().jit_launch(self.key_sums, self.nred, 1, 1, 256, 1, 1, 0,
                         _stream(),
                         [partials.data_ptr(), sums.data_ptr()], [], [])

    def step(self, sums, state, A, B, dt):
        ext().jit_launch(self.key_step, 1, 1, 1, 1, 1, 1, 0, _stream(),
                         [sums.data_ptr(), state.data_ptr()], [],
                         [float(A), float(B), float(dt)])


def get_lap_stage_kernel(map_dict, tmp_instructions, entries, field_args,
                         scalar_names, halo, rank_shape, dx, nf,
                         f_name="f", lap_name="lap_f",
                         name="rk_lapstage", tile=None, nt=True,
                         state_map=None, periodic=(False, False, False),
                         dtype=torch.float64, compile=True):
    return JitLapStage(map_dict, tmp_instructions, entries, field_args,
                       scalar_names, halo, rank_shape, dx, nf,
                       f_name=f_name, lap_name=lap_name, name=name,
                       tile=tile, nt=nt, state_map=state_map,
                       periodic=periodic, dtype=dtype, compile=compile)


def get_lap_reduction_kernel(entries, field_args, scalar_names, halo,
                             rank_shape, dx, nf, f_name="f",
                             lap_name="lap_f", tile=(64, 4, 64),
                             store_lap=True, dtype=torch.float64,
                             compile=True):
    return JitLapReduction(entries, field_args, scalar_names, halo,
                           rank_shape, dx, nf, f_name, lap_name, tile=tile,
                           store_lap=store_lap, dtype=dtype,
                           compile=compile)

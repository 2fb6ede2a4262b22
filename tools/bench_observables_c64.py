"""A/B of the complex64 observable kernels against the torch branch
(PYSTELLA_OBS_C64=0) for PowerSpectra and Projector built on a float32
transform, on one GPU, with the complex128 kernels' time for the same
row (the same objects built on a float64 transform) alongside.

Rows: bin_power, transverse_traceless (in place), tensor_to_pol,
decompose_vector (times_abs_k), and the full PowerSpectra.__call__ (one
scalar field), gw and vector_decomposition, transforms included.  The
three forms run interleaved in one process, --rounds times each, timed
with HIP events after warm-up.  One JSON line per row: the median ms per
call over all rounds for each form, fused/torch, the spread of the round
medians ((max - min) / median), and torch.cuda.max_memory_allocated()
above the allocation held just before the timed calls for the fused and
the torch form.  The torch form forms |f_k|^2 through index_add_, which
takes seconds per spectrum at 512^3, so it gets --torch-calls calls per
round and one warm-up call (default: 2 calls at n >= 512, else --calls);
the line says how many were used.

Run each size in a process of its own, under a time limit:

    timeout 600 python tools/bench_observables_c64.py --n 256 && \\
    timeout 1100 python tools/bench_observables_c64.py --n 512
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HUBBLE = 0.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--torch-calls", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default=None,
                    help="comma-separated subset of the rows")
    p = ap.parse_args()
    if p.torch_calls is None:
        p.torch_calls = 2 if p.n >= 512 else p.calls

    import pystella_amd as ps
    from pystella_amd.fourier import DFT

    if not torch.cuda.is_available():
        sys.exit("bench_observables_c64.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    grid = (p.n,) * 3
    lengths = (5., 3., 7.)
    dk = tuple(2 * np.pi / li for li in lengths)
    dx = tuple(li / n for li, n in zip(lengths, grid))
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)

    def build(dtype):
        fft = DFT(decomp, grid_shape=grid, dtype=dtype, device=dev)
        return (ps.PowerSpectra(decomp, fft, dk, float(np.prod(lengths))),
                ps.Projector(fft, 1, dk, dx), fft)

    gen = torch.Generator(device="cpu").manual_seed(7)
    hij32 = torch.randn((6,) + grid, dtype=torch.float32,
                        generator=gen).to(dev)

    def rows_for(dtype):
        """{row: call} on objects of ``dtype``; the inputs are the same
        numbers for both dtypes."""
        spectra, proj, fft = build(dtype)
        rdtype = torch.float32 if dtype == np.float32 else torch.float64
        cdtype = fft.fk.dtype
        kshape = tuple(fft.shape(True))
        hij = hij32.to(rdtype)
        vec, fx = hij[:3], hij[0]
        hij_k = torch.empty((6,) + kshape, dtype=cdtype, device=dev)
        for mu in range(6):
            fft.dft(hij[mu], hij_k[mu])
        hij_k /= float(p.n)**1.5            # O(1) modes
        tt_k = hij_k.clone()
        outs = torch.empty((3,) + kshape, dtype=cdtype, device=dev)
        return {
            "bin_power": lambda: spectra.bin_power(hij_k[0], k_power=3),
            "transverse_traceless":
                lambda: proj.transverse_traceless(hij=tt_k),
            "tensor_to_pol": lambda: proj.tensor_to_pol(
                plus=outs[0], minus=outs[1], hij=hij_k),
            "decompose_vector": lambda: proj.decompose_vector(
                vector=hij_k[:3], plus=outs[0], minus=outs[1], lng=outs[2],
                times_abs_k=True),
            "call": lambda: spectra(fx),
            "gw": lambda: spectra.gw(hij, proj, HUBBLE),
            "vector_decomposition":
                lambda: spectra.vector_decomposition(vec, proj),
        }

    rows32 = rows_for(np.float32)
    rows64 = rows_for(np.float64)
    names = list(rows32)
    if p.rows:
        names = [r for r in p.rows.split(",") if r in rows32]

    # form -> (calls, PYSTELLA_OBS_C64, per-round calls, warm-up calls)
    forms = {"fused": (rows32, None, p.calls, p.warmup),
             "torch": (rows32, "0", p.torch_calls, 1),
             "c128": (rows64, None, p.calls, p.warmup)}

    for row in names:
        times = {form: [] for form in forms}
        peaks = {form: 0 for form in forms}
        for _ in range(p.rounds):
            for form, (rows, switch, calls, warmup) in forms.items():
                if switch is None:
                    os.environ.pop("PYSTELLA_OBS_C64", None)
                else:
                    os.environ["PYSTELLA_OBS_C64"] = switch
                call = rows[row]
                for _ in range(warmup):
                    call()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ms = []
                for _ in range(calls):
                    start = torch.cuda.Event(enable_timing=True)
                    stop = torch.cuda.Event(enable_timing=True)
                    start.record()
                    call()
                    stop.record()
                    stop.synchronize()
                    ms.append(start.elapsed_time(stop))
                times[form].append(ms)
                peaks[form] = max(peaks[form],
                                  torch.cuda.max_memory_allocated() - base)
        os.environ.pop("PYSTELLA_OBS_C64", None)

        def median(form):
            return statistics.median(t for ms in times[form] for t in ms)

        def spread(form):
            meds = [statistics.median(ms) for ms in times[form]]
            return (max(meds) - min(meds)) / statistics.median(meds)

        out = {"n": p.n, "row": row,
               "fused_ms": round(median("fused"), 4),
               "torch_ms": round(median("torch"), 4),
               "fused_over_torch": round(median("fused") / median("torch"),
                                         5),
               "c128_ms": round(median("c128"), 4),
               "fused_over_c128": round(median("fused") / median("c128"), 4),
               "fused_peak_extra_bytes": int(peaks["fused"]),
               "torch_peak_extra_bytes": int(peaks["torch"]),
               "round_spread": {f: round(spread(f), 4) for f in forms},
               "rounds": p.rounds, "calls_per_round": p.calls,
               "torch_calls_per_round": p.torch_calls}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""A/B of RayleighGenerator's two generators, rng="torch" (a chain of
torch operations) and rng="philox" (one fused HIP kernel), for
init_WKB_fields on one GPU in float64.

Both generators share the transform, the host-side omega_k evaluation
and the two inverse FFTs of a call; the difference is everything between
the uniforms and the stored modes.  They run interleaved in the same
process, --rounds times --calls calls each after warm-up, timed with HIP
events.  One JSON line per (n, rng): the median ms per call over all
rounds, each round's median, and the peak of
torch.cuda.max_memory_allocated() above the allocation held just before
the timed calls (the fields, the transform's buffers and the generator's
|k| array are part of that baseline).

The two generators draw different realisations; nothing is compared.

Usage: python tools/bench_rayleigh.py [--n 256 512] [--rounds 3]
           [--calls 5]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def bench(n, p, dev):
    import pystella_amd as ps
    from pystella_amd.fourier import DFT

    grid = (n,) * 3
    box = (5., 5., 5.)
    dk = tuple(2 * np.pi / li for li in box)
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
    fft = DFT(decomp, grid_shape=grid, dtype=np.float64, device=dev)
    gens = {rng: ps.RayleighGenerator(fft=fft, dk=dk,
                                      volume=float(np.prod(box)),
                                      seed=49279, rng=rng)
            for rng in ("torch", "philox")}
    fx = torch.zeros(grid, dtype=torch.float64, device=dev)
    dfx = torch.zeros(grid, dtype=torch.float64, device=dev)

    def call(rng):
        gens[rng].init_WKB_fields(
            fx, dfx, norm=1.2e-6**2, hubble=0.1,
            omega_k=lambda k: np.sqrt(k**2 + 1.7))

    times = {rng: [] for rng in gens}
    peaks = dict.fromkeys(gens, 0)
    for _ in range(p.rounds):
        for rng in gens:
            for _ in range(p.warmup):
                call(rng)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ms = []
            for _ in range(p.calls):
                start = torch.cuda.Event(enable_timing=True)
                stop = torch.cuda.Event(enable_timing=True)
                start.record()
                call(rng)
                stop.record()
                stop.synchronize()
                ms.append(start.elapsed_time(stop))
            times[rng].append(ms)
            peaks[rng] = max(peaks[rng],
                             torch.cuda.max_memory_allocated() - base)
    assert torch.isfinite(fx).all() and fx.std() > 0
    karray = fft.fk.numel() * 8
    for rng in gens:
        rounds = times[rng]
        print(json.dumps({
            "n": n, "op": "init_WKB_fields", "rng": rng,
            "median_ms": round(statistics.median(
                t for ms in rounds for t in ms), 3),
            "round_median_ms": [round(statistics.median(ms), 3)
                                for ms in rounds],
            "peak_extra_bytes": int(peaks[rng]),
            "peak_extra_real_karrays": round(peaks[rng] / karray, 2),
            "rounds": p.rounds, "calls_per_round": p.calls,
        }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    p = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rayleigh.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for n in p.n:
        bench(n, p, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

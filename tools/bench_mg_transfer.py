"""A/B of the fused multigrid transfer kernels against the torch chain
(PYSTELLA_MG_TRANSFER=0) on one GPU.

The four operations of a FAS cycle (restrict, restrict_and_correct,
interpolate, interpolate_and_correct) are timed with HIP events after
warm-up, both forms interleaved in the same process, --rounds times
--calls calls each, for three configurations: FullWeighting + Linear at
1024^3 -> 512^3 float32 and at 512^3 -> 256^3 float64 (halo 1), and
FullWeighting + Cubic at 512^3 -> 256^3 float64 (halo 2).  One JSON line
per (configuration, operation, form): the median ms per call over all
rounds, each round's median, torch.cuda.max_memory_allocated() above the
allocation held just before the timed calls, and the achieved bytes per
second against the minimum traffic (the fine array read and the coarse
array written once for a restriction, the reverse for a prolongation,
plus one more read of the output for the ``correct`` forms).  Fused rows
also carry fused/torch and the largest difference of their output from
the chain's, relative to the chain's largest magnitude.

Usage: python tools/bench_mg_transfer.py [--rounds 3] [--calls 5]
           [--scale 1]     (--scale 2 halves every extent)
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KNOB = "PYSTELLA_MG_TRANSFER"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    p = ap.parse_args()

    from pystella_amd.multigrid.transfer import (
        CubicInterpolation, FullWeighting, LinearInterpolation)

    if not torch.cuda.is_available():
        sys.exit("bench_mg_transfer.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    # (name, fine interior extent, dtype, halo, prolongation)
    configs = [
        ("fw+linear", 1024, torch.float32, 1, LinearInterpolation),
        ("fw+linear", 512, torch.float64, 1, LinearInterpolation),
        ("fw+cubic", 512, torch.float64, 2, CubicInterpolation),
    ]
    forms = {"fused": None, "torch": "0"}

    def set_form(form):
        if forms[form] is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = forms[form]

    for name, n1, dtype, h, interp in configs:
        n1 //= p.scale
        n2 = n1 // 2
        gen = torch.Generator(device="cpu").manual_seed(7)
        f1 = torch.rand((n1 + 2 * h,) * 3, dtype=dtype,
                        generator=gen).to(dev)
        f2 = torch.rand((n2 + 2 * h,) * 3, dtype=dtype,
                        generator=gen).to(dev)
        f1_0, f2_0 = f1.clone(), f2.clone()
        size = f1.element_size()
        fine, coarse = n1**3 * size, n2**3 * size
        # (operator, the array it writes, minimum bytes moved)
        ops = {
            "restrict": (FullWeighting(h), f2, fine + coarse),
            "restrict_and_correct": (FullWeighting(h, correct=True), f2,
                                     fine + 2 * coarse),
            "interpolate": (interp(h), f1, coarse + fine),
            "interpolate_and_correct": (interp(h, correct=True), f1,
                                        coarse + 2 * fine),
        }
        times = {(op, form): [] for op in ops for form in forms}
        peaks = {key: 0 for key in times}
        results = {}
        for rnd in range(p.rounds):
            for op, (call, out, _) in ops.items():
                for form in forms:
                    set_form(form)
                    for _ in range(p.warmup):
                        call(f1=f1, f2=f2)
                    if rnd == 0:
                        # one call from the same state for both forms
                        f1.copy_(f1_0)
                        f2.copy_(f2_0)
                        call(f1=f1, f2=f2)
                        results[op, form] = out.clone()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    ms = []
                    for _ in range(p.calls):
                        start = torch.cuda.Event(enable_timing=True)
                        stop = torch.cuda.Event(enable_timing=True)
                        start.record()
                        call(f1=f1, f2=f2)
                        stop.record()
                        stop.synchronize()
                        ms.append(start.elapsed_time(stop))
                    times[op, form].append(ms)
                    peaks[op, form] = max(
                        peaks[op, form],
                        torch.cuda.max_memory_allocated() - base)
                    # the correct forms accumulate: start each block of
                    # calls from the same finite values
                    f1.copy_(f1_0)
                    f2.copy_(f2_0)
        os.environ.pop(KNOB, None)

        medians = {key: statistics.median(t for ms in rounds for t in ms)
                   for key, rounds in times.items()}
        for op, (_, _, nbytes) in ops.items():
            for form in forms:
                row = {
                    "config": name, "fine": n1, "coarse": n2,
                    "dtype": str(dtype).replace("torch.", ""), "halo": h,
                    "op": op, "form": form,
                    "median_ms": round(medians[op, form], 4),
                    "round_median_ms": [round(statistics.median(ms), 4)
                                        for ms in times[op, form]],
                    "peak_extra_bytes": int(peaks[op, form]),
                    "min_bytes": nbytes,
                    "achieved_TBps": round(
                        nbytes / (medians[op, form] * 1e-3) / 1e12, 3),
                    "rounds": p.rounds, "calls_per_round": p.calls,
                }
                if form == "fused":
                    row["fused_over_torch"] = round(
                        medians[op, "fused"] / medians[op, "torch"], 4)
                    a, b = results[op, "fused"], results[op, "torch"]
                    row["max_diff_vs_torch"] = (
                        (a - b).abs().max() / b.abs().max()).item()
                print(json.dumps(row), flush=True)
        del f1, f2, f1_0, f2_0, results, ops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

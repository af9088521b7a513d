"""ScaleIntensityRangePercentiles(0.5, 99.5, 0, 1, clip=True) on the headline volumes -- one 512^3 float32 image, and a 4 x 256^3 image channel by channel --
resident in HBM: the order-statistic kernel (csrc/kernels/select.h) plus the apply pass, against the reference's formulation of the same step written out
here with torch and numpy (what monai's percentile() does above 1,000,000 elements: a device-to-host copy, np.percentile per percentile and channel, then
the element-wise apply on the device).  Device events around whole calls, 2 warm-up calls, min and median of --runs timed calls.  Bytes counted for the
product: 3 selection reads + 1 read and 1 write of the apply pass = 5 x 4 bytes per voxel, over the call time, as a fraction of the 6.3 TB/s this chip
copies at.  It is an end-to-end rate of the whole call (seven small launches included), not a kernel's share of peak.  No pass or fail number.

    python tools/bench_percentiles.py [--runs 10] [--ref-runs 3] [--out profiles/percentiles_bench.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BYTES_PER_S = 6.3e12


def reference_formulation(x, lower, upper, b_min, b_max, channel_wise):
    """percentile() above 1,000,000 elements (monai/transforms/utils_pytorch_numpy_unification.py:129-132) + ScaleIntensityRange (intensity/array.py:1005-1009)"""
    outs = []
    for img in (x if channel_wise else [x]):
        host = img.cpu().numpy()
        a_min = torch.as_tensor(np.percentile(host, np.asarray(lower)), dtype=torch.float32, device=x.device)
        a_max = torch.as_tensor(np.percentile(host, np.asarray(upper)), dtype=torch.float32, device=x.device)
        o = (img - a_min) / (a_max - a_min)
        o = o * (b_max - b_min) + b_min
        outs.append(torch.clamp(o, b_min, b_max))
    return torch.stack(outs) if channel_wise else outs[0]


def timed(fn, runs, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        t.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(t))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--ref-runs", type=int, default=3)
    ap.add_argument("--edge", type=int, default=512, help="edge of the single-channel volume; the four-channel one has half of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "percentiles_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if not torch.cuda.is_available():
        with open(args.out, "w") as f:
            f.write("percentile transforms bench: not measured (no GPU available)\n")
        print("not measured (no GPU available)")
        return
    from monai_amd.transforms import ScaleIntensityRangePercentiles

    dev, e = torch.device("cuda"), args.edge
    lines = [f"ScaleIntensityRangePercentiles(0.5, 99.5, 0, 1, clip=True), float32 volumes in HBM (N(100, 300) quantised to 1/8, seeded); device events around whole "
             f"calls, 2 warm-up calls, {args.runs} timed calls (reference formulation: 1 warm-up, {args.ref_runs} timed); device: {torch.cuda.get_device_name(0)}"]
    for what, shape, cw in ((f"1 x {e}^3, whole image", (1, e, e, e), False), (f"4 x {e // 2}^3, channel_wise", (4, e // 2, e // 2, e // 2), True)):
        gen = torch.Generator().manual_seed(5)
        x = (torch.round(torch.randn(shape, generator=gen) * 2400) / 8 + 100).to(dev)
        ours = ScaleIntensityRangePercentiles(0.5, 99.5, 0, 1, clip=True, channel_wise=cw)
        out, ms = timed(lambda: ours(x), args.runs, 2)
        ref, ref_ms = timed(lambda: reference_formulation(x, 0.5, 99.5, 0, 1, cw), args.ref_runs, 1)
        same = bool(torch.equal(out, ref))
        nbytes = 5 * 4 * x.numel()
        rate = nbytes / (min(ms) * 1e-3)
        lines.append(f"{what}: product min {min(ms):.3f} ms, median {statistics.median(ms):.3f} ms per call; {nbytes / 1e9:.2f} GB counted (3 selection reads + apply read + "
                     f"write) -> {rate / 1e12:.2f} TB/s end to end = {rate / HBM_COPY_BYTES_PER_S:.2f} of the {HBM_COPY_BYTES_PER_S / 1e12:.1f} TB/s copy rate")
        lines.append(f"    reference formulation (device -> host copy, np.percentile, device apply): min {min(ref_ms):.1f} ms, median {statistics.median(ref_ms):.1f} ms per call; "
                     f"product is {min(ref_ms) / min(ms):.0f}x faster; outputs bit-identical: {same}")
    lines.append(f"peak device memory: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

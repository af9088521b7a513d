"""DiceMetric on the headline volume: B = 1, K = 5, 512^3 label maps (float32 and uint8) -- the one-pass overlap kernel (csrc/kernels/metrics.h) against the
obvious torch formulation on the same device (one_hot, then sums over the spatial axes).  HIP events, a warm-up, min and median of --runs timed calls each.
Reports the time of the whole ``DiceMetric`` call, of ``ops.overlap_sums`` alone (both kernels + the workspace allocation), the ratio to the torch
formulation, and the kernel's input bytes per second as a fraction of the 8 TB/s HBM peak and of the copy rate measured in the same run.

    python tools/bench_metrics.py [--edge 512] [--classes 5] [--runs 25] [--out profiles/metrics_bench.txt]      (needs an MI355X)
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monai_amd import ops  # noqa: E402
from monai_amd.metrics import DiceMetric  # noqa: E402


def timed(fn, runs, warm=3):
    """milliseconds of every one of `runs` calls (an event pair each), after `warm` untimed ones"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def torch_dice(pred, truth, k):
    """the same scores from one_hot + sums (ignore_empty=True: NaN where the truth has no voxel of the class)"""
    oh_p = torch.nn.functional.one_hot(pred[:, 0].long(), k)
    oh_y = torch.nn.functional.one_hot(truth[:, 0].long(), k)
    axes = tuple(range(1, oh_p.dim() - 1))
    inter, p_o, y_o = (oh_p & oh_y).sum(axes), oh_p.sum(axes), oh_y.sum(axes)
    score = 2.0 * inter.double() / (y_o + p_o).double()      # float64, rounded once: the counts of a 512^3 volume are past float32's 2^24
    return torch.where(y_o > 0, score, torch.full((), float("nan"), dtype=torch.float64, device=pred.device)).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs an MI355X (torch.cuda.is_available() is False)")
    if args.runs < 20:
        raise SystemExit("--runs: at least 20")
    dev, e, k = torch.device("cuda"), args.edge, args.classes
    n = e ** 3
    lines = [f"DiceMetric, B = 1, K = {k}, {e}^3 label maps ({n} voxels); HIP events, 3 warm-up calls, {args.runs} timed calls each; device: {torch.cuda.get_device_name(0)}"]

    # the chip's copy rate in this run: 1 GiB read + 1 GiB written per call
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), args.runs)
    copy_tbps = 2.0 * src.numel() / (min(copy_ms) * 1e-3) / 1e12
    lines.append(f"device copy of 1 GiB (read + write): min {min(copy_ms):.3f} ms, median {statistics.median(copy_ms):.3f} ms -> {copy_tbps:.2f} TB/s (the measured copy rate)")
    del src, dst

    torch.manual_seed(7)      # a prediction that agrees with the truth on about nine voxels in ten
    base_p = torch.randint(0, k, (1, 1, e, e, e), dtype=torch.uint8, device=dev)
    base_y = torch.where(torch.rand((1, 1, e, e, e), device=dev) < 0.9, base_p, torch.randint(0, k, (1, 1, e, e, e), dtype=torch.uint8, device=dev))
    for dtype in (torch.float32, torch.uint8):
        pred, truth = base_p.to(dtype), base_y.to(dtype)
        metric = DiceMetric(num_classes=k, reduction="none")

        def call():
            metric.reset()
            return metric(pred, truth)

        ours, ref = call(), torch_dice(pred, truth, k)
        if not torch.equal(ours, ref):
            raise SystemExit(f"{dtype}: DiceMetric {ours.tolist()} != torch formulation {ref.tolist()}")
        t_call = timed(call, args.runs)
        t_kern = timed(lambda: ops.overlap_sums(pred, truth, k), args.runs)
        t_torch = timed(lambda: torch_dice(pred, truth, k), args.runs)
        nbytes = 2.0 * n * pred.element_size()      # each label map read once
        tbps = nbytes / (min(t_kern) * 1e-3) / 1e12
        lines += [
            f"{str(dtype).replace('torch.', '')} label maps ({nbytes / 1e6:.0f} MB read per call), Dice per class = {[round(v, 6) for v in ours[0].tolist()]} (equal to the torch formulation)",
            f"  DiceMetric.__call__          min {min(t_call):.3f} ms, median {statistics.median(t_call):.3f} ms",
            f"  ops.overlap_sums alone       min {min(t_kern):.3f} ms, median {statistics.median(t_kern):.3f} ms -> {tbps:.2f} TB/s of input = {tbps / 8.0:.2f} of 8 TB/s, "
            f"{tbps / copy_tbps:.2f} of the measured copy rate",
            f"  torch one_hot + sums         min {min(t_torch):.3f} ms, median {statistics.median(t_torch):.3f} ms",
            f"  torch / DiceMetric           {min(t_torch) / min(t_call):.1f} x (min over min), {statistics.median(t_torch) / statistics.median(t_call):.1f} x (median over median)",
        ]
        del pred, truth
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

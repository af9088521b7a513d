"""HD95 + average surface distance + normalised surface Dice on the headline volume: B = 1, K = 5, 512^3 blob-like label maps scored as one-hots, the way
an evaluation loop calls the three metrics after the Dice -- the edge / exact-EDT / surface-record kernels (csrc/kernels/edt.h).  Blob-like masks (the
argmax of smooth random fields), not noise: noise would make every voxel an edge.  HIP events: end to end per metric call and per C entry point (every
launch of an entry between one pair of events), a warm-up, min and median of --runs timed calls.  Where scipy is importable the same distance transform is
also timed on the host with scipy.ndimage.distance_transform_edt, on the cropped edge map of the largest box.  There is no pass or fail number.

    python tools/bench_surface_metrics.py [--edge 512] [--classes 5] [--runs 5] [--out profiles/surface_metrics_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blob_labels(edge, k, seed, dev):
    """[1, 1, edge^3] uint8: argmax of k smooth random fields (coarse noise, trilinear up-sampling)"""
    gen = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, k, 12, 12, 12), generator=gen).to(dev)
    labels = torch.empty((1, 1, edge, edge, edge), dtype=torch.uint8, device=dev)
    for z in range(0, edge, 64):                        # in slabs: the fields are not needed all at once
        zs = torch.linspace(-1, 1, edge, device=dev)[z:z + 64]
        ys = torch.linspace(-1, 1, edge, device=dev)
        grid = torch.stack(torch.meshgrid(zs, ys, ys, indexing="ij")[::-1], dim=-1)[None]
        labels[0, 0, z:z + 64] = torch.nn.functional.grid_sample(coarse, grid, mode="bilinear", align_corners=True).argmax(dim=1)[0].to(torch.uint8)
    return labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if not torch.cuda.is_available():
        with open(args.out, "w") as f:
            f.write("surface metrics bench: not measured (no GPU available)\n")
        print("not measured (no GPU available)")
        return
    from monai_amd import _lib, ops
    from monai_amd.metrics import compute_average_surface_distance, compute_hausdorff_distance, compute_surface_dice

    dev, e, k = torch.device("cuda"), args.edge, args.classes
    lp, ly = blob_labels(e, k, 1, dev), blob_labels(e, k, 2, dev)
    ly = torch.where(torch.rand(ly.shape, device=dev) < 0.5, ly, lp)      # a truth that agrees with the prediction on about half of the volume
    onehot = lambda t: torch.zeros((1, k, e, e, e), device=dev).scatter_(1, t.long(), 1.0)      # noqa: E731
    p, y = onehot(lp), onehot(ly)
    thr = [1.0] * (k - 1)
    lines = [f"surface metrics, B = 1, K = {k} (background excluded), {e}^3 blob-like masks; HIP events, 1 warm-up call, {args.runs} timed calls each; "
             f"device: {torch.cuda.get_device_name(0)}"]

    L = _lib.lib()
    spans, plain_call = [], L.call

    def timed_call(name, *a):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        plain_call(name, *a)
        t.record()
        spans.append((name, s, t))

    calls = {
        "HD95 (compute_hausdorff_distance, percentile=95)": lambda: compute_hausdorff_distance(p, y, percentile=95),
        "ASD (compute_average_surface_distance, symmetric)": lambda: compute_average_surface_distance(p, y, symmetric=True),
        "NSD (compute_surface_dice, threshold 1)": lambda: compute_surface_dice(p, y, thr),
        "ops.surface_records on the uint8 label maps": lambda: ops.surface_records(lp, ly, k, thresholds=thr, first_class=1),
    }
    for what, fn in calls.items():
        result = fn()
        torch.cuda.synchronize()
        wall, per_entry = [], {}
        for _ in range(args.runs):
            spans.clear()
            L.call = timed_call
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            L.call = plain_call
            for name, s, t in spans:
                per_entry.setdefault(name, []).append(0.0)
            acc = {}
            for name, s, t in spans:
                acc[name] = acc.get(name, 0.0) + s.elapsed_time(t)
            for name, ms in acc.items():
                per_entry.setdefault(name + " total", []).append(ms)
        lines.append(f"{what}: end to end (host clock, with the device-to-host reads) min {min(wall):.1f} ms, median {statistics.median(wall):.1f} ms")
        for name, ms in per_entry.items():
            if name.endswith(" total"):
                lines.append(f"    {name[:-6]:<24} min {min(ms):8.2f} ms, median {statistics.median(ms):8.2f} ms per metric call")
        if isinstance(result, torch.Tensor):
            lines.append(f"    result: {[round(v, 4) for v in result[0].tolist()]}")
    boxes = ops.surface_boxes(lp, ly, k, 1)
    lines.append(f"boxes (z0 y0 x0 d h w): {[tuple(int(v) for v in b[:6]) for b in boxes[0]]}")
    try:
        from scipy.ndimage import distance_transform_edt
    except Exception:
        lines.append("scipy.ndimage.distance_transform_edt: not measured (scipy is not importable here)")
    else:
        ci = max(range(k - 1), key=lambda c: int(boxes[0, c, 3]) * int(boxes[0, c, 4]) * int(boxes[0, c, 5]))
        z0, y0, x0, d, h, w = (int(v) for v in boxes[0, ci, :6])
        edges = ops.mask_edges(lp, ly, k, 1)[1][0, ci, z0:z0 + d, y0:y0 + h, x0:x0 + w].cpu().numpy()
        t0 = time.perf_counter()
        distance_transform_edt(~edges)
        lines.append(f"scipy.ndimage.distance_transform_edt on the cropped truth edge map of class {ci + 1} ({d} x {h} x {w}), one CPU thread: "
                     f"{(time.perf_counter() - t0) * 1e3:.0f} ms for ONE of the {2 * (k - 1)} transforms a symmetric metric call needs")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

"""KeepLargestConnectedComponent and FillHoles on the headline volume: a 512^3 five-class uint8 label map (blobs plus speckle, seeded), the way a bundle
cleans the inferer's label map before the metrics -- the connected-component kernels (csrc/kernels/ccl.h).  HIP events per C entry point (every launch
of an entry between one pair of events) and the host clock end to end, a warm-up, min and median of --runs timed calls.  There is no pass or fail
number, and nothing to compare with: the reference's device path needs cuCIM / CuPy and its host path scikit-image.

    python tools/bench_cc_post.py [--edge 512] [--classes 5] [--runs 5] [--out profiles/cc_post_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blob_labels(edge, k, seed, dev, speckle=0.002):
    """[1, edge^3] uint8 with the values 0 .. k - 1: argmax of k smooth random fields (coarse noise, trilinear up-sampling), then `speckle` of the
    voxels set to a random class"""
    gen = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, k, 12, 12, 12), generator=gen).to(dev)
    labels = torch.empty((1, edge, edge, edge), dtype=torch.uint8, device=dev)
    ys = torch.linspace(-1, 1, edge, device=dev)
    for z in range(0, edge, 64):                        # in slabs: the fields are not needed all at once
        grid = torch.stack(torch.meshgrid(ys[z:z + 64], ys, ys, indexing="ij")[::-1], dim=-1)[None]
        labels[0, z:z + 64] = torch.nn.functional.grid_sample(coarse, grid, mode="bilinear", align_corners=True).argmax(dim=1)[0].to(torch.uint8)
    noise = torch.rand(labels.shape, generator=gen).to(dev) < speckle
    rnd = torch.randint(0, k, labels.shape, generator=gen, dtype=torch.uint8).to(dev)
    return torch.where(noise, rnd, labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cc_post_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if not torch.cuda.is_available():
        with open(args.out, "w") as f:
            f.write("connected-component post transforms bench: not measured (no GPU available)\n")
        print("not measured (no GPU available)")
        return
    from monai_amd import _lib
    from monai_amd.transforms import FillHoles, KeepLargestConnectedComponent

    dev, e, k = torch.device("cuda"), args.edge, args.classes
    lab = blob_labels(e, k, 1, dev)
    applied = list(range(1, k))
    lines = [f"connected-component post transforms, one {e}^3 uint8 label map with {k} classes (blobs + speckle, seed 1); HIP events, 1 warm-up call, "
             f"{args.runs} timed calls each; device: {torch.cuda.get_device_name(0)}"]
    L = _lib.lib()
    spans, plain_call = [], L.call

    def timed_call(name, *a):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        plain_call(name, *a)
        t.record()
        spans.append((name, s, t))

    calls = {
        f"KeepLargestConnectedComponent(applied_labels={applied}) [one labelling pass for all classes]": lambda x: KeepLargestConnectedComponent(applied_labels=applied)(x),
        "KeepLargestConnectedComponent() [applied_labels=None: one read of the unique values]": lambda x: KeepLargestConnectedComponent()(x),
        f"KeepLargestConnectedComponent(applied_labels={applied}, independent=False)": lambda x: KeepLargestConnectedComponent(applied_labels=applied, independent=False)(x),
        f"FillHoles(applied_labels={applied}) [one labelling pass per label]": lambda x: FillHoles(applied_labels=applied)(x),
        f"FillHoles(applied_labels={applied}, connectivity=1)": lambda x: FillHoles(applied_labels=applied, connectivity=1)(x),
    }
    for what, fn in calls.items():
        out = fn(lab.clone())
        torch.cuda.synchronize()
        changed = int((out != lab).sum())
        wall, per_entry = [], {}
        for _ in range(args.runs):
            x = lab.clone()
            torch.cuda.synchronize()
            spans.clear()
            L.call = timed_call
            t0 = time.perf_counter()
            fn(x)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            L.call = plain_call
            acc = {}
            for name, s, t in spans:
                acc[name] = acc.get(name, 0.0) + s.elapsed_time(t)
            for name, ms in acc.items():
                per_entry.setdefault(name, []).append(ms)
        lines.append(f"{what}: end to end (host clock) min {min(wall):.1f} ms, median {statistics.median(wall):.1f} ms; voxels changed {changed}")
        for name, ms in per_entry.items():
            lines.append(f"    {name:<16} min {min(ms):8.2f} ms, median {statistics.median(ms):8.2f} ms per call of the transform")
    lines.append(f"peak device memory: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

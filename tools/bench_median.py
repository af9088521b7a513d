"""MedianSmooth at radius 1 (the register selection network) and radius 2 (the general bisection kernel) on the headline volumes -- one 512^3 float32
image and a 4 x 256^3 image -- resident in HBM (csrc/kernels/median.h), against the reference's formulation of the same step written out here in plain
torch (monai/networks/layers/simplelayers.py:441-498: replicate F.pad, a one-hot conv3d with k^3 output channels, torch.median over them) at the largest
of those sizes at which it runs on this device, with the outputs compared (where they differ, the product is compared with the same formulation
evaluated on z-slabs, and the next smaller size is compared in full).  Device events around whole calls, 2 warm-up calls, min and median of --runs
timed calls.  Bytes counted for the product: one read and one write of the volume = 8 bytes per voxel, over the call time, as a fraction of the
6.3 TB/s this chip copies at.  No pass or fail number.

    python tools/bench_median.py [--runs 10] [--ref-runs 2] [--out profiles/median_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BYTES_PER_S = 6.3e12


def reference_formulation(x, radius):
    """median_filter of the reference for a [C, D, H, W] image: every voxel's window becomes k^3 channels, then torch.median over them"""
    k = 2 * radius + 1
    kernel = torch.diag(torch.ones(k ** 3, dtype=x.dtype, device=x.device)).view(k ** 3, 1, k, k, k)
    padded = F.pad(x.reshape(x.shape[0], 1, *x.shape[1:]), pad=[radius] * 6, mode="replicate")
    features = F.conv3d(padded, kernel, padding=0, stride=1)
    return torch.median(features, dim=1)[0].reshape(x.shape)


def equal_in_slabs(x, out, radius, planes=14):
    """`out` against the reference's formulation evaluated on three z-slabs of x (first, middle, last planes, halo included): a check that does not
    need the formulation to work on the whole volume"""
    depth = x.shape[1]
    for z0 in sorted({0, max(0, depth // 2 - planes // 2), max(0, depth - planes)}):
        z1 = min(z0 + planes, depth)
        lo, hi = max(z0 - radius, 0), min(z1 + radius, depth)
        ref = reference_formulation(x[:, lo:hi].contiguous(), radius)
        if not torch.equal(out[:, z0:z1], ref[:, z0 - lo:z1 - lo]):
            return False
    return True


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
    ap.add_argument("--ref-runs", type=int, default=2)
    ap.add_argument("--edge", type=int, default=512, help="edge of the single-channel volume; the four-channel one has half of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if not torch.cuda.is_available():
        with open(args.out, "w") as f:
            f.write("median filter bench: not measured (no GPU available)\n")
        print("not measured (no GPU available)")
        return
    from monai_amd.transforms import MedianSmooth

    dev, e = torch.device("cuda"), args.edge
    out_file = open(args.out, "w")

    class Lines:      # every line goes to the file as it is measured: the reference's formulation may not come back at the larger sizes
        def append(self, line):
            print(line, flush=True)
            out_file.write(line + "\n")
            out_file.flush()

    lines = Lines()
    lines.append(f"MedianSmooth(radius), float32 volumes in HBM (N(100, 300) quantised to 1/8, seeded); device events around whole calls, 2 warm-up calls, {args.runs} timed "
                 f"calls (reference formulation: 1 warm-up, {args.ref_runs} timed); device: {torch.cuda.get_device_name(0)}")
    shapes = ((f"1 x {e}^3", (1, e, e, e)), (f"4 x {e // 2}^3", (4, e // 2, e // 2, e // 2)))
    volumes = {}
    for what, shape in shapes:
        gen = torch.Generator().manual_seed(5)
        volumes[what] = (torch.round(torch.randn(shape, generator=gen) * 2400) / 8 + 100).to(dev)
    for radius in (1, 2):
        ours = MedianSmooth(radius)
        outs = {}
        for what, _ in shapes:
            x = volumes[what]
            outs[what], ms = timed(lambda: ours(x), args.runs, 2)
            nbytes = 8 * x.numel()
            rate = nbytes / (min(ms) * 1e-3)
            lines.append(f"radius {radius}, {what}: product min {min(ms):.3f} ms, median {statistics.median(ms):.3f} ms per call; {nbytes / 1e9:.2f} GB counted (one read + one "
                         f"write) -> {rate / 1e12:.2f} TB/s = {rate / HBM_COPY_BYTES_PER_S:.3f} of the {HBM_COPY_BYTES_PER_S / 1e12:.1f} TB/s copy rate")
        # the reference's formulation at the largest size at which it runs here
        for what, _ in shapes:
            x = volumes[what]
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            try:
                ref, ref_ms = timed(lambda: reference_formulation(x, radius), args.ref_runs, 1)
            except (torch.cuda.OutOfMemoryError, RuntimeError) as err:
                lines.append(f"    radius {radius}, {what}: the reference's formulation did not run ({type(err).__name__}: {str(err).splitlines()[0][:120]})")
                torch.cuda.empty_cache()
                continue
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            same = bool(torch.equal(outs[what], ref))
            del ref
            _, ms = timed(lambda: ours(x), 3, 1)
            lines.append(f"    radius {radius}, {what}: the reference's formulation (replicate pad, one-hot conv3d to {(2 * radius + 1) ** 3} channels, torch.median): min "
                         f"{min(ref_ms):.1f} ms, median {statistics.median(ref_ms):.1f} ms per call, peak memory {peak:.1f} GiB; product is {min(ref_ms) / min(ms):.0f}x "
                         f"faster; outputs bit-identical: {same}")
            if same:
                break
            # seen on the MI355X at 512^3: this torch build's conv3d with a one-hot kernel returns wrong values once the k^3-channel result passes 2^31 elements
            # (it differs from itself evaluated slab by slab); the product is then compared with the slab-wise evaluation, and the next smaller size in full
            lines.append(f"        the formulation evaluated on z-slabs of the same volume (first, middle, last 14 planes): product bit-identical: {equal_in_slabs(x, outs[what], radius)}")
    out_file.close()


if __name__ == "__main__":
    main()

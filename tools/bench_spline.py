"""Spacing(pixdim=1.0, mode=3) and mode=1, both with padding_mode="border", on the headline volumes -- one 512^3 float32 image at 1.5 mm and a 4 x 256^3
image -- resident in HBM (csrc/kernels/spline.h), with the prefilter and the sampler also timed on their own, against the reference's formulation of the
same step on the same box: device -> host copy, scipy.ndimage.map_coordinates per channel on the reference's dense grid, copy back
(monai/transforms/spatial/array.py:2092-2100; with CuPy absent on ROCm the host is where the reference's integer branch can run at all).  Device events
around whole calls, 2 warm-up calls, min and median of --runs timed calls; the host formulation is timed once with time.perf_counter.  Bytes counted for
the prefilter: per pass over an axis the line is read, written, read and written again per pole (32 bytes per coefficient and pole; the first pass reads
fp32: 28), over the call time, as a fraction of the 6.3 TB/s this chip copies at.  No pass or fail number.

    python tools/bench_spline.py [--runs 10] [--out profiles/spline_bench.txt] [--edge 512] [--host-edge 256]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BYTES_PER_S = 6.3e12


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


def host_formulation(x, m, out_size, order):
    """the reference's integer branch for a device tensor where no CuPy exists: copy to the host, map_coordinates per channel, copy back"""
    from scipy import ndimage

    t0 = time.perf_counter()
    img = x.cpu().numpy()
    o = np.stack(list(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_size], indexing="ij")) + [np.ones(tuple(out_size))])
    grid = np.tensordot(np.asarray(m, dtype=np.float64).reshape(3, 4), o, axes=1)
    out = np.stack([ndimage.map_coordinates(c, grid, order=order, mode="nearest") for c in img]).astype(np.float32)
    res = torch.from_numpy(out).to(x.device)
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--edge", type=int, default=512, help="edge of the single-channel volume; the four-channel one has half of it")
    ap.add_argument("--host-edge", type=int, default=256, help="the host formulation is single-threaded scipy (about a microsecond per cubic output voxel): it runs on "
                    "one volume of this edge, next to the product on the same volume; 0 skips it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spline_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if not torch.cuda.is_available():
        with open(args.out, "w") as f:
            f.write("spline resampling bench: not measured (no GPU available)\n")
        print("not measured (no GPU available)")
        return
    from monai_amd import ops
    from monai_amd.data.meta_tensor import MetaTensor
    from monai_amd.transforms import Spacing
    from monai_amd.transforms.spatial.functional import resample_plan, spline_index_matrix

    dev, e = torch.device("cuda"), args.edge
    out_file = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        out_file.write(line + "\n")
        out_file.flush()

    say(f"Spacing(pixdim=1.0, mode=order, padding_mode='border'), float32 volumes in HBM at 1.5 mm (seeded normal data); device events around whole calls, 2 warm-up "
        f"calls, {args.runs} timed calls; device: {torch.cuda.get_device_name(0)}")
    aff = torch.diag(torch.tensor([1.5, 1.5, 1.5, 1.0], dtype=torch.float64))
    h = args.host_edge
    for what, shape, host in ((f"1 x {e}^3", (1, e, e, e), False), (f"4 x {e // 2}^3", (4, e // 2, e // 2, e // 2), False)) + (((f"1 x {h}^3", (1, h, h, h), True),) if h else ()):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dev)
        img = MetaTensor(x, affine=aff)
        for order in (3, 1):
            tr = Spacing(pixdim=1.0, mode=order, padding_mode="border")
            out, ms = timed(lambda: tr(img), args.runs, 2)
            osz = tuple(int(v) for v in out.shape[1:])
            say(f"order {order}, {what} -> {osz[0]} x {osz[1]} x {osz[2]}: Spacing min {min(ms):.3f} ms, median {statistics.median(ms):.3f} ms per call")
            out_size, xform, _, _ = resample_plan(shape[1:], aff, out.meta["affine"], osz)
            m = spline_index_matrix(xform, shape[1:], osz, False).reshape(-1)
            if order > 1 and not host:
                coef, pms = timed(lambda: ops.spline_prefilter(x, order, "nearest"), args.runs, 2)
                nb = coef.numel() * (28 + 32 * 2)          # one pole: three passes, the first reads fp32
                rate = nb / (min(pms) * 1e-3)
                say(f"    prefilter alone ({tuple(coef.shape[1:])} fp64 coefficients per channel): min {min(pms):.3f} ms, median {statistics.median(pms):.3f} ms; "
                    f"{nb / 1e9:.2f} GB counted -> {rate / 1e12:.2f} TB/s = {rate / HBM_COPY_BYTES_PER_S:.3f} of the {HBM_COPY_BYTES_PER_S / 1e12:.1f} TB/s copy rate")
                L = ops._lib.lib()
                dst = torch.empty((shape[0],) + osz, dtype=torch.float32, device=dev)
                mm = (ops.C.c_double * 12)(*[float(v) for v in m])

                def sample():
                    L.call("mh_spline_resample_affine_f32", ops._lib.ptr(coef), shape[0], 3, *shape[1:], ops._lib.ptr(dst), *osz, mm, order, ops.SPLINE_MODES["nearest"], ops._s(x))
                    return dst

                _, sms = timed(sample, args.runs, 2)
                taps = (order + 1) ** 3
                say(f"    sampler alone: min {min(sms):.3f} ms, median {statistics.median(sms):.3f} ms; {taps} fp64 coefficients per output voxel and channel = "
                    f"{dst.numel() * taps * 8 / (min(sms) * 1e-3) / 1e12:.2f} TB/s of cache-line traffic requested, {dst.numel() / (min(sms) * 1e-3) / 1e9:.1f} G outputs/s")
                del coef, dst
            if host:
                ref, host_ms = host_formulation(x, m, osz, order)
                d = (out.as_tensor() - ref).abs().max().item()
                say(f"    the reference's formulation on this box (copy to the host, scipy.ndimage.map_coordinates, copy back): {host_ms:.0f} ms per call = "
                    f"{host_ms / min(ms):.0f}x the product; max |difference| {d:.3g} (max |input| {x.abs().max().item():.3g})")
                del ref
            del out
            torch.cuda.empty_cache()
    out_file.close()


if __name__ == "__main__":
    main()

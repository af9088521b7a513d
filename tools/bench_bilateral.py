"""BilateralFilter (the exact filter, csrc/kernels/bilateral.h) on one 256^3 float32 image and on one 4-channel 128^3 image at spatial sigma 1 (125 taps)
and 2 (1331 taps), resident in HBM.  Device events around whole calls, 2 warm-up calls, min and median of --runs timed calls.  Reported per line: taps
per second (voxels x K^3 / time) and the share of the chip's vector issue time that the inner loop's instruction mix implies -- ISSUE_CYCLES[C] issue
cycles of one SIMD per tap of a wave (from the disassembly: DESIGN.md section 5.13; v_exp_f32 and the packed v_pk_* 4 cycles, the others 2) times the
taps per second over 64 lanes, against 256 CUs x 4 SIMDs x the 2.4 GHz peak clock.  Then max |float32 tile kernel - float64 generic kernel| on a 64^3 crop,
and, where oracle/_ref/monai_ref_C.so is present, the reference's CPU time on that crop with the outputs compared.  No pass or fail number.

    python tools/bench_bilateral.py [--runs 10] [--out profiles/bilateral_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ISSUE_CYCLES = {1: 14.0, 4: 34.6}      # per tap of a wave64 in the 4-tap group loop of bilateral_tile_kernel<C>
SIMDS = 256 * 4
CLOCK_HZ = 2.4e9      # the MI355X's peak engine clock; under load the chip runs below it, so the share is a lower bound


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
    ap.add_argument("--edge", type=int, default=256, help="edge of the single-channel volume; the four-channel one has half of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilateral_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not torch.cuda.is_available():
        with open(args.out, "w") as f:
            f.write("bilateral filter bench: not measured (no GPU available)\n")
        print("not measured (no GPU available)")
        return
    from monai_amd import ops
    from monai_amd.networks.layers import BilateralFilter

    dev, e = torch.device("cuda"), args.edge
    clock = CLOCK_HZ
    out_file = open(args.out, "w")

    def line(text):
        print(text, flush=True)
        out_file.write(text + "\n")
        out_file.flush()

    color_sigma = 0.5
    line(f"BilateralFilter.apply(x, spatial_sigma, {color_sigma}, False), float32 N(0, 1) volumes in HBM (seeded); device events around whole calls, 2 warm-up calls, "
         f"{args.runs} timed calls; device: {torch.cuda.get_device_name(0)}, shares against {clock / 1e9:.1f} GHz")
    shapes = ((f"1 x 1 x {e}^3", (1, 1, e, e, e)), (f"1 x 4 x {e // 2}^3", (1, 4, e // 2, e // 2, e // 2)))
    volumes = {what: torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dev) for what, shape in shapes}
    for sigma in (1.0, 2.0):
        k = ops.bilateral_window(sigma)
        for what, shape in shapes:
            x = volumes[what]
            path = ops.bilateral_filter_path(shape[2:], shape[1], sigma)
            _, ms = timed(lambda: BilateralFilter.apply(x, sigma, color_sigma, False), args.runs, 2)
            taps = x[:, 0].numel() * k ** 3
            rate = taps / (min(ms) * 1e-3)
            share = rate / 64 * ISSUE_CYCLES[shape[1]] / (SIMDS * clock)
            issue = (f"; at {ISSUE_CYCLES[shape[1]]} issue cycles per tap of a wave = {share:.2f} of the vector issue time of {SIMDS} SIMDs" if path == 1 else
                     " (taps from global memory: no instruction count is claimed for this kernel)")
            line(f"sigma {sigma:g} ({k}^3 = {k ** 3} taps), {what}: {'tile' if path == 1 else 'generic'} kernel, min {min(ms):.3f} ms, median {statistics.median(ms):.3f} ms per call; "
                 f"{rate / 1e12:.2f} T taps/s{issue}")
    # float32 tile kernel against the float64 generic kernel (the on-device yardstick) on a 64^3 crop, and the reference's CPU code where it was built
    crop = volumes[shapes[0][0]][:, :, :64, :64, :64].contiguous()
    ref_mod = None
    try:
        from oracle import build_ref

        ref_mod = build_ref.load()
    except Exception as err:      # the compiled reference is optional
        line(f"    oracle/_ref not loaded ({type(err).__name__})")
    for sigma in (1.0, 2.0):
        out32, ms32 = timed(lambda: ops.bilateral_filter(crop, sigma, color_sigma), 3, 1)
        out64, ms64 = timed(lambda: ops.bilateral_filter(crop.double(), sigma, color_sigma), 3, 1)
        diff = float((out32.double() - out64).abs().max())
        line(f"    sigma {sigma:g}, 1 x 1 x 64^3: max |float32 tile - float64 generic| = {diff:.3e} (max |x| = {float(crop.abs().max()):.2f}); float32 min {min(ms32):.3f} ms, "
             f"float64 generic min {min(ms64):.3f} ms")
        if ref_mod is not None:
            host = crop.cpu()
            t0 = time.perf_counter()
            ref32 = ref_mod.bilateral_filter(host, sigma, color_sigma, False)
            dt = time.perf_counter() - t0
            line(f"    sigma {sigma:g}, 1 x 1 x 64^3: the reference's CPU code (bilateralfilter_cpu.cpp, float32) {dt * 1e3:.0f} ms = {dt * 1e3 / min(ms32):.0f}x the product's call; "
                 f"max |product - reference| = {float((out32.cpu() - ref32).abs().max()):.3e}")
    out_file.close()


if __name__ == "__main__":
    main()

"""Golden outputs of the reference's OWN ScaleIntensityRangePercentiles / ClipIntensityPercentiles (monai/transforms/intensity/array.py:1299-1418,
1015-1157; array and dictionary forms) and of its percentile() (monai/transforms/utils_pytorch_numpy_unification.py:104-136) on the cases of
tests/percentile_cases.py, CPU -> tests/golden/percentiles.npz.  Per case id:

    <id>|pct       uint32 [runs][2]: the bits of the fp32 percentile values percentile() returns for the lower / upper percentile of each run
    <id>|out       uint32: the bits of the whole output (small inputs)
    <id>|samp      uint32: the bits of every 997th output value, and  <id>|sum  the fp64 sum of the output (inputs above 100,000 elements)
    <id>|clipvals  float64 [n][2]: meta["clipping_values"] (return_clipping_values=True)

It also measures which form of at::lerp torch.quantile's CPU kernel evaluates (see tests/percentile_cases.py) and refuses to write a golden if
neither the fused nor the unfused form reproduces it.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_percentiles.py"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import monai.transforms as ref  # noqa: E402
from monai.transforms.utils_pytorch_numpy_unification import percentile  # noqa: E402
import percentile_cases as pc  # noqa: E402

warnings.filterwarnings("ignore")


def torch_rule(xs, q, fused):
    n = xs.size
    rank = np.float32(np.float64(q) / 100.0) * np.float32(n - 1)
    lo, hi = np.floor(rank), np.ceil(rank)
    w = np.float32(rank - lo)
    s = np.sort(xs)
    a, b = s[int(lo)], s[int(hi)]
    d = np.float32(b - a)
    base, wa = (a, w) if w < 0.5 else (b, np.float32(w - np.float32(1)))
    if fused:       # the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding only in ties of 2^-29 relative width)
        return np.float32(np.float64(wa) * np.float64(d) + np.float64(base))
    return np.float32(base + np.float32(wa * d))


rng = np.random.default_rng(0)
miss = {True: 0, False: 0}
total = 0
for _ in range(300):
    xs = (rng.standard_normal(int(rng.integers(2, 5000))) * 100).astype(np.float32)
    for q in (0.5, 10, 30, 70, 90, 99.5, 33.3):
        got = torch.quantile(torch.from_numpy(xs), torch.tensor(np.float64(q) / 100.0, dtype=torch.float32)).numpy()
        total += 1
        for fused in (True, False):
            miss[fused] += int(torch_rule(xs, q, fused).view(np.uint32) != got.view(np.uint32))
print(f"torch.quantile over {total} random cases: fused at::lerp differs in {miss[True]}, unfused in {miss[False]}")
assert miss[True] == 0, "torch.quantile's CPU lerp is not the fused form here: the kernel's SEL_LERP_TORCH mode has to follow"

arrays, manifest = {}, []
for case in pc.golden_cases():
    cid = case["id"]
    x = torch.from_numpy(pc.inputs(case["inp"]).copy())
    runs = list(x) if case["kw"].get("channel_wise") else [x]
    qs = pc.pct_args(case)
    pct = np.asarray([[np.float32(percentile(r, q).item()) for q in qs] for r in runs], np.float32)
    assert all(torch.as_tensor(percentile(r, q)).dtype == torch.float32 for r in runs for q in qs)
    arrays[cid + "|pct"] = pct.view(np.uint32)
    out, meta = pc.run_case(ref, case, "cpu")
    o = torch.as_tensor(out).numpy()
    assert o.dtype == np.float32 and o.shape == pc.inputs(case["inp"]).shape, (cid, o.dtype, o.shape)
    if pc.is_large(case["inp"]):
        arrays[cid + "|samp"] = o.reshape(-1)[::pc.STRIDE].view(np.uint32).copy()
        arrays[cid + "|sum"] = np.asarray(o.astype(np.float64).sum())
    else:
        arrays[cid + "|out"] = o.view(np.uint32).copy()
    if case["kw"].get("return_clipping_values"):
        cv = meta["clipping_values"]
        assert isinstance(cv, list) and len(cv) == len(runs), (cid, cv)
        arrays[cid + "|clipvals"] = np.asarray(cv, np.float64)
        assert np.array_equal(arrays[cid + "|clipvals"].astype(np.float32).view(np.uint32), arrays[cid + "|pct"]), cid
    manifest.append(cid)
arrays["manifest"] = np.array(json.dumps(manifest))
path = os.path.join(HERE, "percentiles.npz")
np.savez_compressed(path, **arrays)
print("percentile golden:", len(manifest), "cases,", os.path.getsize(path), "bytes")

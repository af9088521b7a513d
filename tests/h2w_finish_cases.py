"""Seeded launches of the Winograd split convolution (csrc/kernels/conv3d_wino_h2.h) whose results are pinned BIT FOR BIT: which lane
finishes which piece of an output row is free to change, what every piece holds -- and the order the statistics leaves are merged in --
is not.  Shared by the fixture generator (tests/golden/make_golden_h2w_finish.py, run under the SIMT emulator in a checkout of the
commit whose bits are to be kept) and by tests/test_h2w_finish_bits_emu.py."""
import hashlib

import numpy as np
import torch

from monai_amd import ops

import kernel_cases as kc

# (name, form, n, cin, cout, dims): one region; 2 x 2 regions with borders on every side and two cout groups; two z-chunks; the accumulating and the pooling forms
CASES = [
    ("plain_1x32x32_3x4x16", "plain", 1, 32, 32, (3, 4, 16)),
    ("plain_2x32x64_5x8x32", "plain", 2, 32, 64, (5, 8, 32)),
    ("plain_1x32x32_24x4x16", "plain", 1, 32, 32, (24, 4, 16)),
    ("acc_1x32x32_3x4x32", "acc", 1, 32, 32, (3, 4, 32)),
    ("pool_1x32x32_4x8x16", "pool", 1, 32, 32, (4, 8, 16)),
]
FULL_LIMIT = 64 * 1024      # tensors above this many bytes are kept as the SHA-256 of their bytes


def inputs(seed, n, cin, cout, dims, with_old=False):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin) + tuple(dims), generator=gen)
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(27.0 * cin)
    b = torch.randn(cout, generator=gen) * 0.1
    nrm = kc._with_bounds(x, kc._rand_nrm(n, cin, gen), loosen=float(np.sqrt(np.prod(dims))))
    old = torch.randn((n, cout) + tuple(dims), generator=gen) * 2.0 if with_old else None
    return x, w, b, nrm, old


def run_case(device, form, n, cin, cout, dims, seed=4100):
    """-> {tensor name: CPU tensor} of one launch; every output buffer is NaN-prefilled so that an unwritten piece shows"""
    cfg = ops.conv3d_k3_h2w_config()
    x, w, b, nrm, old = inputs(seed + cout + dims[0] + dims[2], n, cin, cout, dims, with_old=form == "acc")
    packed = ops.conv3d_k3_pack(cfg, w.to(device))
    tiles = ops.conv3d_k3_stat_tiles(cfg, *dims)
    stats = torch.full((n, cout, tiles, 3), float("nan"), device=device)
    res = {}
    if form == "acc":
        out = old.clone().to(device)
        ops.conv3d_k3(cfg, x.to(device), nrm.to(device), packed, b.to(device), out, stats, accumulate=True)
    elif form == "pool":
        out = torch.full((n, cout) + tuple(dims), float("nan"), device=device)
        pdims = tuple(v // 2 for v in dims)
        pmx = torch.full((n, cout) + pdims, float("nan"), device=device)
        pmn = torch.full((n, cout) + pdims, float("nan"), device=device)
        ops.conv3d_k3_pool(cfg, x.to(device), nrm.to(device), packed, b.to(device), out, stats, pmx, pmn)
        res["pool_max"], res["pool_min"] = pmx.cpu(), pmn.cpu()
    else:
        out = torch.full((n, cout) + tuple(dims), float("nan"), device=device)
        ops.conv3d_k3(cfg, x.to(device), nrm.to(device), packed, b.to(device), out, stats)
    res["out"], res["stats"] = out.cpu(), stats.cpu()
    return res


def pinned(name, t):
    """what the fixture keeps of a tensor: (key, array) -- statistics always in full, other tensors above FULL_LIMIT as a digest"""
    a = np.ascontiguousarray(t.numpy())
    assert a.dtype == np.float32
    if name != "stats" and a.nbytes > FULL_LIMIT:
        return name + ".sha256", np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
    return name, a.view(np.uint32)      # as bit patterns: NaNs compare like everything else


def all_cases(device):
    got = {}
    for cname, form, n, cin, cout, dims in CASES:
        for tname, t in run_case(device, form, n, cin, cout, dims).items():
            key, arr = pinned(tname, t)
            got[f"{cname}/{key}"] = arr
    return got

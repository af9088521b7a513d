"""Seeded launches of the Winograd split convolution (csrc/kernels/conv3d_wino_h2.h) that walk every split of its march into generic head blocks, steady blocks and
generic tail blocks: a chunk of depth d runs ceil((d + 3) / 3) blocks of three iterations, the first two generic and the last one or two (every block with a plane
that does not exist), so depth <= 7 has no steady block, 8-10 one, 11-13 two, and depths 8..13 cover every remainder of the chunk's length mod 3 behind a steady block.
Their results are pinned BIT FOR BIT to the commit
before the march was split (tests/golden/h2w_march_parent.npz, written by tests/golden/make_golden_h2w_march.py under the SIMT emulator in a checkout of that commit)
and run on the MI355X by tests/test_h2w_march_gpu.py.  Inputs and the NaN prefill of every output buffer are those of tests/h2w_finish_cases.py."""
import h2w_finish_cases as hc

REGION = (4, 16)      # one workgroup region
# (name, form, n, cin, cout, dims)
CASES = (
    [(f"plain_d{d}", "plain", 1, 32, 32, (d,) + REGION) for d in (2, 5, 6, 7, 8, 9, 10, 11, 12, 13)]
    + [(f"acc_d{d}_w32", "acc", 1, 32, 32, (d, 4, 32)) for d in (8, 9, 10)]
    + [(f"pool_d{d}", "pool", 1, 32, 32, (d,) + REGION) for d in (2, 8, 10, 12)]
    # two chunks of 14 planes with halo planes inside the volume
    + [("plain_d28_two_chunks", "plain", 1, 32, 32, (28,) + REGION), ("pool_d28_two_chunks", "pool", 1, 32, 32, (28,) + REGION)]
    # 2 x 2 regions with borders on every side, two cout groups, two samples
    + [("plain_2x32x64_d10_2x2_regions", "plain", 2, 32, 64, (10, 8, 32))]
)


def all_cases(device):
    got = {}
    for cname, form, n, cin, cout, dims in CASES:
        for tname, t in hc.run_case(device, form, n, cin, cout, dims).items():
            key, arr = hc.pinned(tname, t)
            got[f"{cname}/{key}"] = arr
    return got

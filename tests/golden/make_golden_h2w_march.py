"""Bits of the Winograd split convolution (conv3d_k3_h2w_kernel) under the SIMT emulator, for tests/test_h2w_march_bits_emu.py: the outputs, the statistics
records, the pooled maxima and minima of the launches in tests/h2w_march_cases.py.  h2w_march_parent.npz holds the bits of the commit BEFORE the march was split
into generic head and tail blocks and steady blocks: the split march has to reproduce them.  Run from THIS checkout, naming a checkout of the commit whose bits
are to be kept -- its kernels, emulator and package are used, only the list of launches comes from here:
    git worktree add <dir> <commit>
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_h2w_march.py --tree <dir> [output.npz]
Without --tree it writes the bits of this checkout itself (to compare two commits by hand; not for the fixture)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
args = sys.argv[1:]
tree = os.path.dirname(os.path.dirname(HERE))
if args and args[0] == "--tree":
    tree = os.path.abspath(args[1])
    args = args[2:]
# the kernels, tests/emu, emu_backend, kernel_cases, h2w_finish_cases and monai_amd of `tree`; h2w_march_cases from this checkout
sys.path[:0] = [os.path.join(tree, "tests"), tree]
sys.path.append(os.path.dirname(HERE))
from emu_backend import emu_backend  # noqa: E402
from h2w_march_cases import all_cases  # noqa: E402

dst = args[0] if args else os.path.join(HERE, "h2w_march_parent.npz")
with emu_backend():
    out = all_cases("cpu")
np.savez_compressed(dst, **out)
print("h2w march golden of", tree, ":", len(out), "arrays,", os.path.getsize(dst), "bytes")

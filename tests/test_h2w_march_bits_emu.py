"""The march of conv3d_k3_h2w_kernel (csrc/kernels/conv3d_wino_h2.h) is split into generic blocks at a chunk's head and end and steady blocks between them, in which
nothing is tested per plane; the staging conversion, the pooled stores and the pooling exchange changed their instructions with it.  None of that may change a bit:
the outputs, statistics records, pooled maxima and minima of the seeded launches in tests/h2w_march_cases.py -- every head / steady / tail split, two chunks, borders --
are BIT FOR BIT those of the commit before the split (tests/golden/h2w_march_parent.npz, written there by tests/golden/make_golden_h2w_march.py under the same SIMT
emulator)."""
import os

import numpy as np
import pytest

import h2w_finish_cases as hc
import h2w_march_cases as mc


@pytest.fixture(scope="module")
def parent(golden_dir):
    with np.load(os.path.join(golden_dir, "h2w_march_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_covers_every_case(parent):
    want = set()
    for cname, form, *_ in mc.CASES:
        want |= {f"{cname}/stats"} | ({f"{cname}/pool_max", f"{cname}/pool_min"} if form == "pool" else set())
        assert f"{cname}/out" in parent or f"{cname}/out.sha256" in parent
    assert want <= set(parent) and len(parent) == len(want) + len(mc.CASES)
    assert all(parent[f"{c[0]}/stats"].dtype == np.uint32 for c in mc.CASES)      # the records in full, as bit patterns


def test_cases_cover_every_split():
    """a one-chunk volume of depth d runs blocks at p = -1, 2, 5, ... <= d + 1; block p is steady from the third on while its last plane p + 2 exists (<= d - 1)"""
    steady = {d: max((d - 2) // 3 - 1, 0) for d in (c[5][0] for c in mc.CASES if c[1] == "plain" and c[5][1:] == mc.REGION and c[5][0] < 28)}
    assert {0, 1, 2} <= set(steady.values())
    assert {d % 3 for d, s in steady.items() if s >= 1} == {0, 1, 2}


@pytest.mark.parametrize("cname,form,n,cin,cout,dims", mc.CASES, ids=[c[0] for c in mc.CASES])
def test_h2w_march_bits(emu, parent, cname, form, n, cin, cout, dims):
    got = hc.run_case("cpu", form, n, cin, cout, dims)
    assert not any(bool(t.isnan().any()) for t in got.values()), "a piece was left unwritten"
    keys = []
    for tname, t in got.items():
        key, arr = hc.pinned(tname, t)
        exp = parent[f"{cname}/{key}"]
        keys.append(key)
        assert arr.shape == exp.shape and arr.dtype == exp.dtype, key
        bad = int(np.count_nonzero(arr != exp))
        assert bad == 0, f"{cname}/{key}: {bad} of {arr.size} words differ from the parent commit's"
    assert sorted(keys) == sorted(k.split("/", 1)[1] for k in parent if k.startswith(cname + "/"))

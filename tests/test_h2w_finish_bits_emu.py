"""The finishing step of conv3d_k3_h2w_kernel (csrc/kernels/conv3d_wino_h2.h) may hand its pieces to other lanes -- whole 64-byte output rows per lane quad -- but
every piece keeps its value and the statistics leaves keep their merge tree: the outputs, statistics records, pooled maxima and minima of the seeded launches in
tests/h2w_finish_cases.py are BIT FOR BIT those of the commit before the re-mapping (tests/golden/h2w_finish_parent.npz, written there by
tests/golden/make_golden_h2w_finish.py under the same SIMT emulator)."""
import os

import numpy as np
import pytest

import h2w_finish_cases as hc


@pytest.fixture(scope="module")
def parent(golden_dir):
    with np.load(os.path.join(golden_dir, "h2w_finish_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_covers_every_case(parent):
    want = set()
    for cname, form, *_ in hc.CASES:
        want |= {f"{cname}/stats"} | ({f"{cname}/pool_max", f"{cname}/pool_min"} if form == "pool" else set())
        assert f"{cname}/out" in parent or f"{cname}/out.sha256" in parent
    assert want <= set(parent) and len(parent) == len(want) + len(hc.CASES)
    assert all(parent[f"{c[0]}/stats"].dtype == np.uint32 for c in hc.CASES)      # the records in full, as bit patterns


@pytest.mark.parametrize("cname,form,n,cin,cout,dims", hc.CASES, ids=[c[0] for c in hc.CASES])
def test_h2w_finish_bits(emu, parent, cname, form, n, cin, cout, dims):
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

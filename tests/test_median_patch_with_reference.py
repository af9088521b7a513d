"""Drop-in check of the median filter against the real MONAI (only where /root/reference exists): after ``monai_amd.patch.install()`` the reference's
six names are the product's objects, a reference ``Compose`` with ``MedianSmoothd`` reproduces a golden case on the emulator (which stands in for the
device) without a fall-through, a float64 tensor and a custom ``kernel=`` fall through and equal the unpatched reference's results, and
``uninstall()`` restores the originals."""
import os
import sys

import numpy as np
import pytest
import torch

REF = "/root/reference"
pytestmark = [pytest.mark.fallthrough, pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "monai")), reason="reference MONAI not available here")]


@pytest.fixture()
def monai_ref():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import monai

    yield monai
    import monai_amd.patch as patch

    patch.uninstall()
    sys.path.remove(REF)


def test_patched_names_compose_and_fall_through(monai_ref, emu, monkeypatch):
    import monai.networks.layers as ref_l
    import monai.networks.layers.simplelayers as ref_sl
    import monai.transforms as ref_t
    import monai.transforms.intensity.array as ref_a
    import monai.transforms.intensity.dictionary as ref_d
    import median_cases as mc
    import monai_amd.networks.layers as our_l
    import monai_amd.patch as patch
    import monai_amd.transforms as ours
    from monai.bundle import ConfigParser
    from monai_amd import _fallback

    monkeypatch.delenv("MONAI_AMD_NO_FALLTHROUGH", raising=False)
    t_names = ["MedianSmooth", "MedianSmoothd", "MedianSmoothD", "MedianSmoothDict"]
    displaced = {n: getattr(ref_t, n) for n in t_names}
    displaced_l = {n: getattr(ref_sl, n) for n in ("MedianFilter", "median_filter")}
    case = next(c for c in mc.golden_cases() if c["id"] == "smoothd-2ch-9x70-r1")
    img = torch.from_numpy(mc.inputs(case).copy())
    x64 = torch.from_numpy(mc.data("normal", (1, 4, 5, 6), 3)).double()
    x32 = x64.float()
    cross = torch.zeros(7, 1, 3, 3, 3)          # a custom kernel: the 7 voxels of the 3-D cross instead of the 27 of the box
    for i, (z, y, x) in enumerate(((1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2))):
        cross[i, 0, z, y, x] = 1.0
    pure64 = ref_sl.MedianFilter(1)(x64)
    pure_cross = ref_sl.median_filter(x32, kernel=cross)

    done = patch.install()
    for n in t_names:
        assert getattr(ref_t, n) is getattr(ours, n) and getattr(ref_d if n != "MedianSmooth" else ref_a, n) is getattr(ours, n), n
    for n in ("MedianFilter", "median_filter"):
        assert getattr(ref_sl, n) is getattr(our_l, n) and getattr(ref_l, n) is getattr(our_l, n), n
    for full in ("monai.transforms.intensity.array.MedianSmooth", "monai.transforms.intensity.dictionary.MedianSmoothd",
                 "monai.networks.layers.simplelayers.MedianFilter", "monai.networks.layers.simplelayers.median_filter"):
        assert full in done, full
    before = len(_fallback.fell_through())
    pipe = ref_t.Compose([ref_t.MedianSmoothd(keys="img", radius=1)])
    assert isinstance(pipe.transforms[0], ours.MedianSmoothd)
    out = pipe({"img": img.clone()})["img"]
    assert mc.same_as_reference(torch.as_tensor(out).numpy(), mc.golden()[case["id"]])
    assert isinstance(ConfigParser({"pre": {"_target_": "MedianSmoothd", "keys": "img", "radius": 1}}).get_parsed_content("pre"), ours.MedianSmoothd)
    assert len(_fallback.fell_through()) == before      # all of it served by the kernel
    # float64 and a custom kernel are the reference's
    got64 = ref_l.MedianFilter(1)(x64)
    # (the reference's MedianFilter.forward calls the module's median_filter -- the product's while installed -- which hands the call on once more)
    after64 = len(_fallback.fell_through())
    assert got64.dtype == torch.float64 and torch.equal(got64, pure64) and after64 > before
    assert _fallback.fell_through()[before][0] == "MedianFilter.forward"
    got_cross = ref_l.median_filter(x32, kernel=cross)
    assert torch.equal(got_cross, pure_cross) and len(_fallback.fell_through()) == after64 + 1 and _fallback.fell_through()[-1][0] == "median_filter"
    assert not torch.equal(got_cross, ref_l.median_filter(x32))
    patch.uninstall()
    for n, obj in displaced.items():
        assert getattr(ref_t, n) is obj, n
    for n, obj in displaced_l.items():
        assert getattr(ref_sl, n) is obj and getattr(ref_l, n) is obj, n
    assert np.array_equal(ref_sl.MedianFilter(1)(x64).numpy(), pure64.numpy())

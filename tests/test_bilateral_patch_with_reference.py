"""Drop-in check of the exact bilateral filter against the real MONAI (only where /root/reference exists): after ``monai_amd.patch.install()``
``monai.networks.layers.BilateralFilter`` and ``monai.networks.layers.filtering.BilateralFilter`` are the product's autograd function, it reproduces a
golden case on the emulator (which stands in for the device) without a fall-through, and ``uninstall()`` restores the reference's."""
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


def test_patched_names_and_uninstall(monai_ref, emu, monkeypatch):
    import monai.networks.layers as ref_l
    import monai.networks.layers.filtering as ref_f
    import bilateral_cases as bc
    import monai_amd.networks.layers as our_l
    import monai_amd.patch as patch
    from monai_amd import _fallback

    monkeypatch.delenv("MONAI_AMD_NO_FALLTHROUGH", raising=False)
    displaced = ref_f.BilateralFilter
    assert displaced is ref_l.BilateralFilter and displaced is not our_l.BilateralFilter
    done = patch.install()
    assert ref_f.BilateralFilter is our_l.BilateralFilter and ref_l.BilateralFilter is our_l.BilateralFilter
    assert "monai.networks.layers.filtering.BilateralFilter" in done
    before = len(_fallback.fell_through())
    case = next(c for c in bc.golden_cases() if c["id"] == "chan-2d-c3")
    g = bc.golden(case["file"])
    out = ref_l.BilateralFilter.apply(torch.from_numpy(bc.inputs(case).copy()), case["ss"], case["cs"], False).numpy()
    tol, _ = bc.bound(case, g[case["id"] + "/ref32"].view(np.float32), g[case["id"] + "/ref64"])
    assert float(np.abs(out.astype(np.float64) - g[case["id"] + "/ref64"]).max()) <= tol
    assert len(_fallback.fell_through()) == before      # served by the kernel
    with pytest.raises(RuntimeError, match="fast_approx=False"):
        ref_l.BilateralFilter.apply(torch.zeros(1, 1, 4, 4))
    patch.uninstall()
    assert ref_f.BilateralFilter is displaced and ref_l.BilateralFilter is displaced

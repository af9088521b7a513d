"""Drop-in check of the percentile intensity transforms against the real MONAI (only where /root/reference exists): after
``monai_amd.patch.install()`` the reference's names are the product's classes, a reference ``Compose`` with ``ScaleIntensityRangePercentilesd`` reproduces
the pure-reference run bit for bit on the emulator (which stands in for the device) without a fall-through, a bundle-style ``_target_`` resolves to the
product class, and ``uninstall()`` restores the originals."""
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


def test_patched_compose_reproduces_the_reference_run(monai_ref, emu, monkeypatch):
    import monai.transforms as ref_t
    import monai.transforms.intensity.array as ref_a
    import monai.transforms.intensity.dictionary as ref_d
    import percentile_cases as pc
    import monai_amd.patch as patch
    import monai_amd.transforms as ours
    from monai.bundle import ConfigParser
    from monai_amd import _fallback

    monkeypatch.delenv("MONAI_AMD_NO_FALLTHROUGH", raising=False)
    names = [b + s for b in ("ScaleIntensityRangePercentiles", "ClipIntensityPercentiles") for s in ("", "d", "D", "Dict")]
    displaced = {n: getattr(ref_t, n) for n in names}
    for n, text in pc.SIGNATURES.items():           # the literal the API test compares with IS the reference's signature
        assert pc.signature_text(displaced[n]) == text and pc.signature_text(getattr(ours, n)) == text, n
    img = torch.from_numpy(pc.inputs("small").copy())

    def pipeline():
        return ref_t.Compose([
            ref_t.ScaleIntensityRangePercentilesd(keys="img", lower=0.5, upper=99.5, b_min=0, b_max=1, clip=True, channel_wise=True),
            ref_t.ClipIntensityPercentilesd(keys="img", lower=10, upper=90),
        ])

    pure = pipeline()({"img": img.clone()})["img"]
    assert type(pipeline().transforms[0]) is displaced["ScaleIntensityRangePercentilesd"]
    doc = torch.tensor(pc.DOC_IMAGE, dtype=torch.float32)
    pure_soft = ref_t.ClipIntensityPercentiles(30, 70, 10.0)(doc)

    done = patch.install()
    for n in names:
        assert getattr(ref_t, n) is getattr(ours, n), n
        assert getattr(ref_d if n[-1] in "dDt" else ref_a, n) is getattr(ours, n), n
    assert "monai.transforms.intensity.dictionary.ScaleIntensityRangePercentilesd" in done and "monai.transforms.intensity.array.ClipIntensityPercentiles" in done
    before = len(_fallback.fell_through())
    pipe = pipeline()
    assert isinstance(pipe.transforms[0], ours.ScaleIntensityRangePercentilesd) and isinstance(pipe.transforms[1], ours.ClipIntensityPercentilesd)
    out = pipe({"img": img.clone()})["img"]
    assert type(out) is type(pure) and np.array_equal(torch.as_tensor(out).numpy().view(np.uint32), torch.as_tensor(pure).numpy().view(np.uint32))
    assert len(_fallback.fell_through()) == before      # all of it served by the kernels
    # a bundle names the component by its short name
    parser = ConfigParser({"pre": {"_target_": "ScaleIntensityRangePercentilesd", "keys": "img", "lower": 0.5, "upper": 99.5, "b_min": 0, "b_max": 1, "clip": True},
                           "clipper": {"_target_": "ClipIntensityPercentilesd", "keys": "img", "lower": 1, "upper": 99}})
    assert isinstance(parser.get_parsed_content("pre"), ours.ScaleIntensityRangePercentilesd)
    assert isinstance(parser.get_parsed_content("clipper"), ours.ClipIntensityPercentilesd)
    # the soft clip is the reference's: the constructor hands the object over
    soft = ref_t.ClipIntensityPercentiles(30, 70, 10.0)(doc)
    assert len(_fallback.fell_through()) > before and type(soft) is type(pure_soft) and torch.equal(torch.as_tensor(soft), torch.as_tensor(pure_soft))
    patch.uninstall()
    for n, obj in displaced.items():
        assert getattr(ref_t, n) is obj, n

"""The reference's OWN unittest module for the exact bilateral filter (tests/networks/layers/filtering/test_bilateral_precise.py), run unmodified with
``monai_amd._C`` standing in for the compiled extension ``monai._C`` and the product's ``BilateralFilter`` patched in (tests/ref_suite_runner.py
--compiled; see tests/test_reference_suites_emu.py: the same runner, the same rules).  ``BilateralFilterTestCaseCpuPrecise`` runs both of its methods
over every row -- the hard-coded expectations at atol=1e-5 and ``gradcheck(..., raise_exception=False)`` -- and the CUDA class is skipped by its own
decorator where there is no device.  RUN / SKIPPED are the counts the same module gives over the unpatched reference with the reference's own compiled
module (oracle/_ref) standing in for ``monai._C`` (measured); the product has to give the same, with kernel launches.
Skipped where the reference checkout is absent (the GPU box)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TESTS = "/root/reference/tests"
MODULE = "networks/layers/filtering/test_bilateral_precise.py"
RUN, SKIPPED = 32, 16      # 8 rows x (2 CPU methods + 2 CUDA methods); the CUDA class's 16 skipped without a device


def _monai_importable() -> bool:
    if not os.path.isdir(REF_TESTS):
        return False
    sys.path.insert(0, "/root/reference")
    try:
        import monai  # noqa: F401
    except Exception:
        return False
    finally:
        sys.path.remove("/root/reference")
    return True


pytestmark = [pytest.mark.skipif(not _monai_importable(), reason="the reference checkout (/root/reference) is not present"), pytest.mark.fallthrough]


def test_reference_bilateral_precise_module_passes_over_the_product():
    path = os.path.join(REF_TESTS, MODULE)
    if not os.path.exists(path):
        pytest.skip(f"{MODULE} is not part of this reference checkout")
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("MONAI_AMD_NO_FALLTHROUGH", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_suite_runner.py"), path, "--compiled"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (p.stdout[-1500:], p.stderr[-3000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["failures"] == 0 and res["errors"] == 0 and p.returncode == 0, (res["failed"], p.stderr[-4000:])
    assert res["run"] == RUN and res["skipped"] == SKIPPED, res
    assert res["kernel_launches"] > 0, res
    assert not res["fell_through"], res

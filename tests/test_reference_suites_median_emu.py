"""The reference's OWN unittest modules for MedianFilter and MedianSmooth(d), run unmodified over the product classes (see
tests/test_reference_suites_emu.py: the same runner, the same rules).  MODULES holds the number of tests the reference itself passes in each
module here (measured by running the module over the unpatched reference); the product has to pass the same, with kernel launches in each.
Skipped where the reference checkout is absent (the GPU box)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TESTS = "/root/reference/tests"

# (module, tests the reference itself passes there)
MODULES = [("networks/layers/test_median_filter.py", 4), ("transforms/test_median_smooth.py", 3), ("transforms/test_median_smoothd.py", 4)]


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


@pytest.mark.parametrize("module,n_tests", MODULES, ids=[m for m, _ in MODULES])
def test_reference_median_module_passes_over_the_product(module, n_tests):
    path = os.path.join(REF_TESTS, module)
    if not os.path.exists(path):
        pytest.skip(f"{module} is not part of this reference checkout")
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("MONAI_AMD_NO_FALLTHROUGH", None)        # the fall-through to the reference is part of what is tested
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_suite_runner.py"), path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, (p.stdout[-1500:], p.stderr[-3000:])
    res = json.loads(lines[-1][len("RESULT "):])
    assert res["failures"] == 0 and res["errors"] == 0 and p.returncode == 0, (res["failed"], p.stderr[-4000:])
    assert res["run"] == n_tests and res["skipped"] == 0, res
    assert res["kernel_launches"] > 0, res

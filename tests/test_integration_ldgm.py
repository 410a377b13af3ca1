"""CPU: the configure path integration/ultragrid_mi355x.patch gives the ldgm_gpu library.  The LDGM GPU section of the patched configure.ac
(from its `ldgm_gpu=no` to its ENSURE_FEATURE_PRESENT) is run by sh with add_module and ENSURE_FEATURE_PRESENT stood in for, under the
combinations that matter: --enable-ldgm-gpu without CUDA must now succeed when libug_mi355x was found, and change nothing otherwise."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PATCH = os.path.join(ROOT, "integration", "ultragrid_mi355x.patch")

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "configure.ac")) or shutil.which("patch") is None,
                                reason="needs the reference's configure.ac and patch(1)")


@pytest.fixture(scope="module")
def section(tmp_path_factory):
    d = tmp_path_factory.mktemp("cfg")
    shutil.copy(os.path.join(REF, "configure.ac"), d / "configure.ac")
    subprocess.run(["patch", "-s", "-p1", "-i", PATCH], cwd=d, check=True)
    txt = (d / "configure.ac").read_text()
    start = txt.index('if test "${ldgm_gpu_req?}" != no && test "${ldgm?}" = yes &&')
    end = txt.index("ENSURE_FEATURE_PRESENT([$ldgm_gpu_req], [$ldgm_gpu]", start)
    end = txt.index("\n", end)
    assert txt.index("found_ug_mi355x=no") < start  # the library is probed before the LDGM section
    body = txt[start:end]
    body = re.sub(r"ENSURE_FEATURE_PRESENT\(\[\$ldgm_gpu_req\], \[\$ldgm_gpu\], \[[^]]*\]\)",
                  'if test "$ldgm_gpu_req" = yes && test "$ldgm_gpu" != yes; then echo "ENSURE FAILED"; exit 1; fi', body)
    return body


def _run(body, **env):
    pre = "add_module() { echo \"ADD $1 $2\"; }\nldgm_gpu=no\nCUDA_LIB=-lcudart\nCUDA_COMMON_OBJ=\nWORD_LEN=64\nsystem=Linux\n"
    pre += "".join(f"{k}={v}\n" for k, v in env.items())
    r = subprocess.run(["sh", "-c", pre + body + '\necho "ldgm_gpu=$ldgm_gpu"'], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_enable_ldgm_gpu_without_cuda_uses_the_mi355x_library(section):
    rc, out = _run(section, ldgm_gpu_req="yes", ldgm="yes", FOUND_CUDA="no", found_ug_mi355x="yes", UG_MI355X_LIB="-lug_mi355x")
    assert rc == 0 and "ldgm_gpu=yes" in out
    assert "ADD ldgm_gpu src/rtp/ldgm_gpu_mi355x.o" in out


def test_without_the_library_it_still_fails_as_before(section):
    rc, out = _run(section, ldgm_gpu_req="yes", ldgm="yes", FOUND_CUDA="no", found_ug_mi355x="no")
    assert rc == 1 and "ENSURE FAILED" in out


def test_cuda_build_keeps_the_cuda_library(section):
    rc, out = _run(section, ldgm_gpu_req="auto", ldgm="yes", FOUND_CUDA="yes", found_ug_mi355x="yes")
    assert rc == 0 and "ldgm_gpu=yes" in out
    assert "ldgm_gpu_mi355x" not in out and out.count("ADD ldgm_gpu") == 1


def test_disabled_or_no_ldgm_adds_nothing(section):
    for env in (dict(ldgm_gpu_req="no", ldgm="yes"), dict(ldgm_gpu_req="auto", ldgm="no")):
        rc, out = _run(section, FOUND_CUDA="no", found_ug_mi355x="yes", **env)
        assert rc == 0 and "ADD" not in out and "ldgm_gpu=no" in out

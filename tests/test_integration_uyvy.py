"""CPU: what integration/ultragrid_mi355x.patch and install.sh do for `-c uyvy` and the reference's DXT module names.  The MI355X module
section of the patched configure.ac is run by sh (add_module and AC_DEFINE stood in for) under the decisions configure makes for uyvy, rtdxt
and cuda_dxt; the installed uyvy_mi355x.cpp is compiled where install.sh put it, and the stand-in names are registered only where the
patch's macros say the reference's module is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PATCH = os.path.join(ROOT, "integration", "ultragrid_mi355x.patch")

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "configure.ac")) or shutil.which("patch") is None,
                                reason="needs the reference tree and patch(1)")


@pytest.fixture(scope="module")
def section(tmp_path_factory):
    d = tmp_path_factory.mktemp("cfg")
    shutil.copy(os.path.join(REF, "configure.ac"), d / "configure.ac")
    subprocess.run(["patch", "-s", "-p1", "-i", PATCH], cwd=d, check=True)
    txt = (d / "configure.ac").read_text()
    start = txt.index('if test "${found_ug_mi355x?}" = yes\nthen\n        ug_mi355x=yes')
    end = txt.index("ENSURE_FEATURE_PRESENT([$ug_mi355x_req]", start)
    # the section comes after configure has decided uyvy, rtdxt and cuda_dxt
    assert txt.index("\nuyvy=no\n") < start and txt.index("\nrtdxt=no\n") < start and txt.index("\ncuda_dxt=no\n") < start
    return txt[start:end]


def _run(body, **env):
    pre = "add_module() { echo \"ADD $1 $2\"; }\nAC_DEFINE() { echo \"DEFINE $1\"; }\nUG_MI355X_LIB=-lug_mi355x\n"
    pre += "".join(f"{k}={v}\n" for k, v in env.items())
    body = re.sub(r"AC_DEFINE\(\[(\w+)\], \[1\], \[[^]]*\]\)", r"AC_DEFINE \1", body)
    r = subprocess.run(["sh", "-c", pre + body], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_headless_build_takes_all_three_names(section):
    out = _run(section, found_ug_mi355x="yes", uyvy="no", rtdxt="no", cuda_dxt="no")
    assert "ADD vcompress_uyvy_mi355x src/video_compress/uyvy_mi355x.o" in out
    for m in ("MI355X_NO_UYVY_COMPRESS", "MI355X_NO_RTDXT", "MI355X_NO_CUDA_DXT"):
        assert f"DEFINE {m}" in out, m


def test_build_with_the_reference_modules_changes_nothing_of_theirs(section):
    out = _run(section, found_ug_mi355x="yes", uyvy="yes", rtdxt="yes", cuda_dxt="yes")
    assert "ADD vcompress_uyvy_mi355x" in out and "DEFINE" not in out
    out = _run(section, found_ug_mi355x="yes", uyvy="yes", rtdxt="no", cuda_dxt="yes")
    assert out.count("DEFINE") == 1 and "DEFINE MI355X_NO_RTDXT" in out


def test_without_the_library_nothing_is_added(section):
    out = _run(section, found_ug_mi355x="no", uyvy="no", rtdxt="no", cuda_dxt="no")
    assert "ADD" not in out and "DEFINE" not in out


def _compile(tmp_path, src, defines):
    ug = tmp_path / "UltraGrid"
    if not ug.exists():
        ug.mkdir()
        shutil.copy(os.path.join(REF, "configure.ac"), ug / "configure.ac")
        subprocess.run(["sh", os.path.join(ROOT, "integration", "install.sh"), str(ug)], check=True, capture_output=True)
    cfg = tmp_path / ("cfg_" + "_".join(defines or ["none"]))
    cfg.mkdir(exist_ok=True)
    (cfg / "config.h").write_text("".join(f"#define {d} 1\n" for d in defines))
    obj = cfg / "m.o"
    r = subprocess.run(["g++", "-std=gnu++20", "-c", "-DHAVE_CONFIG_H", "-D_GNU_SOURCE", "-msse4.1", "-I", str(cfg), "-I", os.path.join(REF, "src"),
                        str(ug / src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return obj.read_bytes()


def test_installed_uyvy_module_compiles_and_takes_uyvy_only_when_told(tmp_path):
    plain = _compile(tmp_path, "src/video_compress/uyvy_mi355x.cpp", [])
    assert b"\0uyvy_mi355x\0" in plain and b"\0uyvy\0" not in plain
    assert b"\0uyvy\0" in _compile(tmp_path, "src/video_compress/uyvy_mi355x.cpp", ["MI355X_NO_UYVY_COMPRESS"])


def test_installed_dxt_module_takes_the_reference_names_only_when_told(tmp_path):
    plain = _compile(tmp_path, "src/video_compress/dxt_mi355x.cpp", [])
    assert b"\0rtdxt\0" not in plain and b"\0cuda_dxt\0" not in plain
    both = _compile(tmp_path, "src/video_compress/dxt_mi355x.cpp", ["MI355X_NO_RTDXT", "MI355X_NO_CUDA_DXT"])
    assert b"\0rtdxt\0" in both and b"\0cuda_dxt\0" in both
    one = _compile(tmp_path, "src/video_compress/dxt_mi355x.cpp", ["MI355X_NO_RTDXT"])
    assert b"\0rtdxt\0" in one and b"\0cuda_dxt\0" not in one

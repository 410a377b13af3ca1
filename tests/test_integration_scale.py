"""CPU: what integration/ultragrid_mi355x.patch and install.sh do for `-p scale`, and the stand-in's names in UltraGrid's registry.  The patched
configure.ac's scale section is run by sh (add_module and AC_DEFINE stood in for) under the decisions configure makes for `scale`; the installed
scale_mi355x.c is compiled where install.sh put it; the registry is listed through oracle/_ref/ug_vopp_harness (the module object linked in).  No GPU: nothing here initialises the module."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PATCH = os.path.join(ROOT, "integration", "ultragrid_mi355x.patch")
OUT = os.path.join(ROOT, "oracle", "_ref")

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "configure.ac")) or shutil.which("patch") is None,
                                reason="needs the reference tree and patch(1)")


@pytest.fixture(scope="module")
def section(tmp_path_factory):
    d = tmp_path_factory.mktemp("cfg")
    shutil.copy(os.path.join(REF, "configure.ac"), d / "configure.ac")
    subprocess.run(["patch", "-s", "-p1", "-i", PATCH], cwd=d, check=True)
    txt = (d / "configure.ac").read_text()
    start = txt.index("# -p scale without GL")
    end = txt.index("\nfi\n", start) + 4
    # after configure has decided scale (and after the detection of the library)
    assert txt.index("\nscale=no\n") < txt.index("ENSURE_FEATURE_PRESENT([$scale_req], [$scale], [Scale not found])") < start
    assert txt.index("found_ug_mi355x=") < start
    return txt[start:end]


def _run(body, **env):
    pre = "add_module() { echo \"ADD $1 $2\"; }\nAC_DEFINE() { echo \"DEFINE $1\"; }\nUG_MI355X_LIB=-lug_mi355x\n"
    pre += "".join(f"{k}={v}\n" for k, v in env.items())
    body = re.sub(r"AC_DEFINE\(\[(\w+)\], \[1\], \[[^]]*\]\)", r"AC_DEFINE \1", body)
    r = subprocess.run(["sh", "-c", pre + body], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_headless_build_takes_the_scale_name(section):
    out = _run(section, found_ug_mi355x="yes", scale="no")
    assert "ADD vo_pp_scale_mi355x src/vo_postprocess/scale_mi355x.o" in out and "DEFINE MI355X_NO_SCALE_PP" in out


def test_gl_build_keeps_the_reference_module(section):
    out = _run(section, found_ug_mi355x="yes", scale="yes")
    assert "ADD vo_pp_scale_mi355x" in out and "DEFINE" not in out


def test_without_the_library_nothing_is_added(section):
    out = _run(section, found_ug_mi355x="no", scale="no")
    assert "ADD" not in out and "DEFINE" not in out


def _compile(tmp_path, defines):
    ug = tmp_path / "UltraGrid"
    if not ug.exists():
        ug.mkdir()
        shutil.copy(os.path.join(REF, "configure.ac"), ug / "configure.ac")
        subprocess.run(["sh", os.path.join(ROOT, "integration", "install.sh"), str(ug)], check=True, capture_output=True)
        assert (ug / "src" / "vo_postprocess" / "scale_mi355x.c").read_bytes() == open(os.path.join(ROOT, "ultragrid_amd", "module", "vo_pp_scale_mi355x.c"), "rb").read()
        assert (ug / "src" / "vo_postprocess" / "mi355x_receiver.h").exists()
        assert (ug / "src" / "vo_postprocess" / "mi355x_gpu_state.h").exists()
    cfg = tmp_path / ("cfg_" + "_".join(defines or ["none"]))
    cfg.mkdir(exist_ok=True)
    (cfg / "config.h").write_text("".join(f"#define {d} 1\n" for d in defines))
    obj = cfg / "m.o"
    r = subprocess.run(["gcc", "-std=gnu2x", "-c", "-DHAVE_CONFIG_H", "-D_GNU_SOURCE", "-I", str(cfg), "-I", os.path.join(REF, "src"),
                        str(ug / "src" / "vo_postprocess" / "scale_mi355x.c"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return obj.read_bytes()


def test_installed_module_compiles_and_takes_scale_only_when_told(tmp_path):
    plain = _compile(tmp_path, [])
    assert b"\0scale_mi355x\0" in plain and b"\0scale\0" not in plain
    assert b"\0scale\0" in _compile(tmp_path, ["MI355X_NO_SCALE_PP"])


@pytest.mark.skipif(not os.path.exists(os.path.join(OUT, "ug_vopp_harness")), reason="oracle/_ref/ug_vopp_harness not built")
def test_registry_lists_the_stand_in_under_both_names():
    r = subprocess.run([os.path.join(OUT, "ug_vopp_harness"), "list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    names = r.stdout.split()
    assert "scale_mi355x" in names and "scale" in names and "same=1" in names


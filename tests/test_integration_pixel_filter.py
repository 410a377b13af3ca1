"""CPU: what integration/ultragrid_mi355x.patch and install.sh do for the colour / mirror filters: the patched configure.ac's block is run by sh
(add_module stood in for), the installed pixel_mi355x.c is compiled where install.sh put it, and the registry of oracle/_ref/ug_cfilter_harness
lists the six names, as capture filters and as postprocessors, beside the reference's.  No GPU: nothing here initialises the module."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PATCH = os.path.join(ROOT, "integration", "ultragrid_mi355x.patch")
OUT = os.path.join(ROOT, "oracle", "_ref")
NAMES = ["matrix_mi355x", "matrix2_mi355x", "gamma_mi355x", "grayscale_mi355x", "mirror_mi355x", "flip_mi355x"]

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "configure.ac")) or shutil.which("patch") is None,
                                reason="needs the reference tree and patch(1)")


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    d = tmp_path_factory.mktemp("cfg")
    shutil.copy(os.path.join(REF, "configure.ac"), d / "configure.ac")
    subprocess.run(["patch", "-s", "-p1", "-i", PATCH], cwd=d, check=True)
    txt = (d / "configure.ac").read_text()
    deint = txt.index("# the de-interlacers on the MI355X")
    start = txt.index("# the colour / mirror filters on the MI355X")
    assert txt.index("found_ug_mi355x=") < deint < txt.index("\nfi\n", deint) < start, "a block of its own, behind the de-interlacers' closing fi"
    return txt[start: txt.index("\nfi\n", start) + 4]


def _run(body, **env):
    pre = "add_module() { echo \"ADD $1 $2 $3\"; }\nUG_MI355X_LIB=-lug_mi355x\n" + "".join(f"{k}={v}\n" for k, v in env.items())
    r = subprocess.run(["sh", "-c", pre + body], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_module_is_added_with_the_library(block):
    assert _run(block, found_ug_mi355x="yes").strip() == "ADD vcapfilter_pixel_mi355x src/capture_filter/pixel_mi355x.o -lug_mi355x"


def test_without_the_library_nothing_is_added(block):
    assert _run(block, found_ug_mi355x="no") == ""


def test_installed_module_compiles_where_install_put_it(tmp_path):
    ug = tmp_path / "UltraGrid"
    ug.mkdir()
    shutil.copy(os.path.join(REF, "configure.ac"), ug / "configure.ac")
    subprocess.run(["sh", os.path.join(ROOT, "integration", "install.sh"), str(ug)], check=True, capture_output=True)
    src = ug / "src" / "capture_filter" / "pixel_mi355x.c"
    assert src.read_bytes() == open(os.path.join(ROOT, "ultragrid_amd", "module", "capture_filter_pixel_mi355x.c"), "rb").read()
    for h in ("mi355x_receiver.h", "mi355x_gpu_state.h", "ug_codec_map.h"):
        assert (ug / "src" / "capture_filter" / h).exists()
    (tmp_path / "config.h").write_text("")
    obj = tmp_path / "m.o"
    r = subprocess.run(["gcc", "-std=gnu2x", "-Wall", "-Wextra", "-c", "-DHAVE_CONFIG_H", "-D_GNU_SOURCE", "-I", str(tmp_path), "-I", os.path.join(REF, "src"),
                        str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    code = obj.read_bytes()
    for name in NAMES:
        assert b"\0" + name.encode() + b"\0" in code, name


@pytest.mark.skipif(not os.path.exists(os.path.join(OUT, "ug_cfilter_harness")), reason="oracle/_ref/ug_cfilter_harness not built")
def test_registry_lists_the_names_beside_the_reference_modules():
    r = subprocess.run([os.path.join(OUT, "ug_cfilter_harness"), "list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    pp, cf = (part.split() for part in r.stdout.split("capture filters:"))
    for name in NAMES:
        assert name in pp and name[: -len("_mi355x")] in pp, name  # no name is taken over
        assert name in cf and name[: -len("_mi355x")] in cf, name

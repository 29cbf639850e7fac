"""What the three classifier setters refuse, pack and bind, without a GPU: warpdemux_amd/csrc/wdx_model_image.h swept by
tests/host/model_image_check.cpp -- built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded).  The program binds every packed image against its own host bytes, reads every value back
through the kernels' records and compares it with the caller's arrays, asserts that every piece is aligned, inside the image
and apart from the others, and makes every refusal of the setters once, message for message (its own header lists the sweep).
The library's setters run the same three functions; what they add needs a device (tests/test_gpu_model_install.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "model_image_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("model_image") / "model_image_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    return out


def test_images_and_refusals_over_the_model_domain_under_sanitizers(exe):
    run = subprocess.run([exe], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    words = run.stderr.decode().split()
    assert words[-1] == "refusals" and words[-3] == "models", run.stderr[-200:]
    # 15 k x 4 rotations x 4 (thresholds, label map) SVMs alone; 16 + 18 + 19 refusals at least
    assert int(words[-4]) > 2000 and int(words[-2]) >= 53, run.stderr[-200:]


def test_the_header_is_host_only_and_owns_the_records():
    """no HIP and nothing of the context in the header; the records the kernels take are stated there and nowhere else"""
    hdr = open(os.path.join(CSRC, "wdx_model_image.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    common = open(os.path.join(CSRC, "wdx_common.h")).read()
    assert '#include "wdx_model_image.h"' in common
    for rec in ("SvmDev", "MlpDev", "BoostTree", "BoostSplit", "BoostDev"):
        assert "struct %s {" % rec in hdr and "struct %s {" % rec not in common, rec

"""CPU: what the host-buffer matchers of okvfe::HipFrontend (okvis2_amd/host/okvfe_frontend.hpp) hand to the library.

tests/cpp/host_marshalling_main.cpp drives matchStereo, matchMotionStereo, matchToMap, matchToMapPooled,
matchToMapUninitialised and verifyRecognisedPlace of a two-camera rig (camera 1 an okvfe_camera_ext with
OKVFE_DIST_RADTAN8) against the recording stand-in tests/cpp/fake_okvfe.cpp, compiled with
-fsanitize=address,undefined: frames of 0, 1 and 5 keypoints, tables of 0, 1 and 3 landmarks, optional vectors empty
and given; every scalar and every array of each call, the camera and the context, the outputs on their way back; and
every ill-formed call (a length one short or one long, a camera index equal to numCameras(), an empty descBegin) must
throw OKVFE_ERR_INVALID_ARGUMENT before the library is reached.  A second build against tests/mock checks the
AssociationHook route of okvfe::HipViFrontend.  No GPU and no libokvfe.so are involved."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the sanitizer runtimes are linked into the program, so it runs the same whatever else the loader brings along)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
HOOK = ["-DOKVFE_WITH_OPENCV=1", "-DOKVFE_WITH_OKVIS=1", "-DOKVFE_MOCK_OKVIS=1", "-I" + os.path.join(ROOT, "tests", "mock")]


@pytest.fixture(scope="module")
def sanitizer_links(tmp_path_factory):
    d = tmp_path_factory.mktemp("asan_probe")
    src = d / "probe.cpp"
    src.write_text("int main(){}\n")
    r = subprocess.run(["g++"] + SANITIZE + ["-o", str(d / "probe"), str(src)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link with " + SANITIZE[0] + " here: " + r.stderr[-200:])


@pytest.mark.parametrize("name,extra", [("host_buffer_matchers", []), ("association_hook_route", HOOK)])
def test_marshalling_under_sanitizers(sanitizer_links, tmp_path, name, extra):
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-pthread"] + SANITIZE + extra + [
        "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "host_marshalling_main.cpp"),
        os.path.join(ROOT, "tests", "cpp", "fake_okvfe.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # (a wrapper that indexes its mutexes with an unchecked camera index can block for ever: the limit ends that run)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stderr == "", out.stderr  # no sanitizer report, no failure line
    assert out.stdout.rstrip().endswith(", 0 failures")


def test_scenes_of_the_gpu_comparison_meet_their_floors(oracle):
    """tests/cpp_matcher_scenes.py: the scenes test_gpu_cpp_matchers.py runs through the C++ mirror hold enough matched,
    accepted, pooled and back-projection-dependent rows for the comparison to mean something (oracle alone)"""
    import cpp_matcher_scenes as S
    fig = S.check_floors()
    print(fig)

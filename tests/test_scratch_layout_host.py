"""CPU: okvis2_amd/csrc/scratch_layout.h (ScratchLayout: where a host-array entry point puts each of its arrays inside the
context's scratch buffer) compiled by g++ into a host program, tests/cpp/scratch_layout_main.cpp -- the header includes
nothing of HIP.  The program lays out sequences of the sizes 0, 1, 255, 256, 257 and 700 * 48 and checks that every offset
is a multiple of 256, that regions are pairwise disjoint, that an empty region has an offset of its own and a byte, that
total() covers the last region, and that the offsets are those of the `take` lambda the entry points carried before (it
is restated there: three lines).  Built plainly and with -fsanitize=address,undefined; both runs exit 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sequences the program runs: the empty one, every 1-, 2- and 3-tuple of the six sizes (the triples twice: bare and with
# a tail), the 720 orders of all six, and 4 x 3 shapes of the stereo matcher
SEQUENCES = 1 + 6 + 36 + 2 * 216 + 720 + 12


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_layout_program(tmp_path, flags):
    exe = tmp_path / "scratch_layout_main"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + ROOT, *flags, "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", "scratch_layout_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    word, sequences, regions = out.stdout.split()
    assert word == "ok" and int(sequences) == SEQUENCES and int(regions) > 6 * SEQUENCES // 2


def test_header_is_free_of_hip():
    text = open(os.path.join(ROOT, "okvis2_amd", "csrc", "scratch_layout.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<cstddef>"], includes

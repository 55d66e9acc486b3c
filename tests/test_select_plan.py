"""CPU: which selection kernel launch_select runs for the shipped configurations (lazy_plan, csrc/k_select.hip) and the
dynamic LDS it asks for, as the lab build exports them on plain integers (okvfe_lab_select_plan: it derives the
occupancy grid as a context does).  tests/test_gpu_select_keys.py asserts with the same export that its cases run
select_lazy_kernel.  EuRoC's figure is pinned: with 240 B of static LDS, six images per CU leave it about 500 bytes."""
import ctypes as C
import os
import subprocess

from okvis2_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_LIB = os.path.join(ROOT, "okvis2_amd", "libokvfe_lab.so")
CU_LDS, STATIC_LDS = 160 * 1024, 240  # per CU; select_lazy_kernel<true>'s static part as built


def plan(cfg):
    assert os.path.exists(LAB_LIB), "libokvfe_lab.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lab = C.CDLL(LAB_LIB)  # (loads without a GPU, like the product library)
    out = (C.c_int32 * 3)()
    lab.okvfe_lab_select_plan(int(cfg.w), int(cfg.h), C.c_float(cfg.uniformity_radius), int(cfg.max_kpts),
                              int(cfg.max_kpts), out)
    return dict(zip(("array", "list", "lds"), out))


def test_shipped_configurations_and_their_lds():
    got = {}
    for name in sorted(n for n in dir(synth) if n.endswith("_config")):
        cfg = getattr(synth, name)()
        got[cfg.name] = plan(cfg)
        assert got[cfg.name]["array"] + got[cfg.name]["list"] == 1, (cfg.name, got[cfg.name])
        assert 0 < got[cfg.name]["lds"] <= 159 * 1024
    assert got["mono640"]["list"] == 1  # the fine grid: linked lists
    assert all(p["array"] == 1 for n, p in got.items() if n != "mono640"), got
    # EuRoC, the flagship: six images per CU (the kernel's six waves per SIMD) must keep fitting
    assert got["euroc"]["lds"] == 26560 and 6 * (got["euroc"]["lds"] + STATIC_LDS) <= CU_LDS
    assert got["tumvi1024"]["lds"] == 34048


def test_plan_function_is_exported_by_the_lab_build_only():
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "okvfe_lab_select_plan" in exported(LAB_LIB)
    assert "okvfe_lab_select_plan" not in exported(os.path.join(ROOT, "okvis2_amd", "libokvfe.so"))

"""CPU: the one function that picks the descriptor kernel of a call (describe_route, csrc/capi_detect.cpp) against a
restatement of the rules it replaced.

Before the call plan existed the choice was spread over two places, and the restatement below is written from them as
they stood in the commit before (95d24c6):

* `aware_box_for_call` (capi_detect.cpp:151-160): may describe_aware_kernel serve the call, and what is the set-up told
  about the pattern's samples beyond 64;
* `launch_describe` (k_describe.hip:821-877): the guard that clears `all_camera_aware` for scale-invariant extraction
  and unaligned images (:844-845) BEFORE `aware_extra_box >= 0` is tested (:850), the describe_rot_kernel test
  (:857-858) and the final if-chain over the describe_kernel instantiations (:864-875);
* their caller `describe_stage` (capi_detect.cpp:550-555): all_camera_aware = the batch's all_aware, rot_fast =
  none_aware && pattern_rot_ok.

The lab build exports the function on plain integers (okvfe_lab_describe_route); no A/B knob is involved (the two that
touch the route, OKVFE_DESC_WAVES and OKVFE_DESC_GENERIC, are applied by launch_describe afterwards).  The sweep is the
full product of the inputs: nothing is left out, combinations no entry point can produce included."""
import ctypes as C
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_LIB = os.path.join(ROOT, "okvis2_amd", "libokvfe_lab.so")

# DescribeRoute (okvfe_internal.h)
AWARE_BATCHED, ROT, W4_AWARE_WIDE, W4_WIDE, W4_ALL_MODES, W5_AWARE, W6_AWARE = range(7)
AWARE_MAX_EXTRA = 6  # kAwareMaxExtra

FIELDS = ("all_aware", "none_aware", "aware_fast", "wide_patches", "box_class", "rot_ok", "extra", "scale_invariant",
          "n_layers", "w", "h", "aligned")


def parent_aware_box(f):
    """aware_box_for_call, capi_detect.cpp:151-160 of the parent"""
    if (not f["all_aware"] or not f["aware_fast"] or f["box_class"] > 1 or f["extra"] > AWARE_MAX_EXTRA
            or f["scale_invariant"] or f["n_layers"] != 1 or f["w"] % 4 != 0 or not f["aligned"] or f["w"] >= 4096
            or f["h"] >= 4096):
        return -1
    return 0 if f["extra"] == 0 else ((f["extra"] << 8) | (4 if f["box_class"] == 0 else 9))


def parent_route(f):
    """launch_describe, k_describe.hip:843-875 of the parent, with the arguments describe_stage gave it"""
    box = parent_aware_box(f)
    all_camera_aware = f["all_aware"]
    rot_fast = f["none_aware"] and f["rot_ok"]
    scales = f["scale_invariant"]
    dword = f["w"] % 4 == 0 and f["aligned"]
    if scales or not dword:                                         # :844-845
        all_camera_aware = False
    if all_camera_aware and box >= 0 and f["box_class"] <= 1:       # :850
        return AWARE_BATCHED
    if rot_fast and f["box_class"] == 0 and not scales and dword:   # :857-858
        return ROT
    if f["box_class"] == 1 and not scales:                          # :864-865
        return W4_AWARE_WIDE if all_camera_aware else W4_WIDE
    if not all_camera_aware or f["box_class"] != 0:                 # :866-870
        return W4_ALL_MODES
    return W5_AWARE if f["wide_patches"] else W6_AWARE              # :871-875


def _sweep():
    tf = (False, True)
    for (all_aware, none_aware, aware_fast, wide_patches, box_class, rot_ok, extra, scale_invariant, n_layers, w, h,
         aligned) in itertools.product(tf, tf, tf, tf, (0, 1, 2), tf, (0, 1, 6, 7), tf, (1, 3),
                                       (752, 750, 4096, 4098), (480, 4096), tf):
        yield dict(zip(FIELDS, (all_aware, none_aware, aware_fast, wide_patches, box_class, rot_ok, extra,
                                scale_invariant, n_layers, w, h, aligned)))


def test_route_truth_table_matches_the_rules_it_replaced():
    assert os.path.exists(LAB_LIB), "libokvfe_lab.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lab = C.CDLL(LAB_LIB)  # (loads without a GPU, like the product library: tests/test_capi_host.py)
    fn = lab.okvfe_lab_describe_route
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    seen, n, bad = {}, 0, []
    for f in _sweep():
        arr = (C.c_int32 * 12)(*[int(f[k]) for k in FIELDS])
        box = C.c_int32(-99)
        route = fn(arr, C.byref(box))
        want = (parent_route(f), parent_aware_box(f))
        if (route, box.value) != want and len(bad) < 10:
            bad.append((f, (route, box.value), want))
        seen[route] = seen.get(route, 0) + 1
        n += 1
    assert not bad, bad
    assert n == 2 ** 4 * 3 * 2 * 4 * 2 * 2 * 4 * 2 * 2
    # the sweep reaches every kernel form launch_describe can launch
    assert sorted(seen) == list(range(7)), seen


def test_route_function_is_exported_by_the_lab_build_only():
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "okvfe_lab_describe_route" in exported(LAB_LIB)
    product = exported(os.path.join(ROOT, "okvis2_amd", "libokvfe.so"))
    assert "okvfe_lab_describe_route" not in product
    assert not [s for s in product if s.startswith("okvfe_lab_")], "the product library exports a lab symbol"

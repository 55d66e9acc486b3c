"""CPU: the scenes of tests/unaligned_cases.py reach what they are for.  Everything here comes from the CPU oracle and
from the lab build's two planning exports (okvfe_lab_select_plan, okvfe_lab_describe_route) -- no kernel runs.

* the census: at least CENSUS_FLOOR candidates / kept keypoints in every place where the generic kernels' index
  arithmetic changes (rim columns and rows, x = w - 3 inside a partial quad, x >= 256 and >= 512, first and last rows
  of the row blocks, keypoints the extractor drops at the right and bottom rim);
* every (w, h, radius, max keypoints) takes the selection form it is filed under, every describe case takes kAllModes or
  kWideBoxes once the image is unaligned;
* the stride residues of the odd batches, the layer widths of the scale-space shapes;
* the scenes can see the mistakes they are for: a score that is off by one, or one missing rim candidate, changes the
  oracle's own output."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import describe_scenes as DS
import unaligned_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_LIB = os.path.join(ROOT, "okvis2_amd", "libokvfe_lab.so")
CSRC = os.path.join(ROOT, "okvis2_amd", "csrc")
DENSE_ROUTES = ("kAllModes", "kWideBoxes")


def lab():
    assert os.path.exists(LAB_LIB), "libokvfe_lab.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    return C.CDLL(LAB_LIB)  # (loads without a GPU, like the product library)


def select_form(w, h, radius, max_kpts):
    out = (C.c_int32 * 3)()
    lab().okvfe_lab_select_plan(int(w), int(h), C.c_float(radius), int(max_kpts), int(max_kpts), out)
    return "array" if out[0] else ("list" if out[1] else "grid")


def describe_route(w, h, aligned, aware, pattern_key="default", jac=None, fu=1.0, scale_invariant=False, steer=0.0):
    """describe_route (csrc/capi_detect.cpp) on the facts a context derives, as describe_scenes.predicted_route states
    them -- with the alignment of the image pointer as an input"""
    p = DS.pattern(pattern_key)
    slow, large = DS.camera_stats(DS.steer(jac, steer), fu, p) if aware else (0.0, 0.0)
    facts = dict(all_aware=aware, none_aware=not aware, aware_fast=slow * 10 <= 1, wide_patches=large * 5 > 2,
                 box_class=DS.box_class(p), rot_ok=p.border <= 29 and p.n_points - 64 <= 6,
                 extra=max(p.n_points - 64, 0), scale_invariant=scale_invariant, n_layers=1, w=w, h=h, aligned=aligned)
    fn = lab().okvfe_lab_describe_route
    fn.restype = C.c_int32
    box = C.c_int32()
    return DS.ROUTE_NAMES[fn((C.c_int32 * 12)(*[int(v) for v in facts.values()]), C.byref(box))]


def test_tile_constants_are_those_of_the_kernels():
    harris = open(os.path.join(CSRC, "k_harris.hip")).read()
    nms = open(os.path.join(CSRC, "k_nms.hip")).read()
    assert int(re.search(r"constexpr int kTH = (\d+);", harris).group(1)) == U.K_TH
    assert int(re.search(r"#define OKVFE_K1_WPB (\d+)", harris).group(1)) == U.K_WAVES_PER_BLOCK
    assert "constexpr int kWavesPerBlock = OKVFE_K1_WPB;" in harris
    assert int(re.search(r"constexpr int kGenIters = (\d+);", nms).group(1)) == U.K_GEN_ITERS
    assert U.NMS_BLOCK_ROWS == 32 and U.HARRIS_BLOCK_ROWS == 128


def test_shapes_cover_the_index_arithmetic():
    widths = [w for w, _ in U.ODD_SHAPES]
    assert sorted(widths) == sorted(w for ws in U.WIDTH_CLASSES.values() for w in ws)
    assert all(w % 4 for w in widths) and all(w % 4 for w, _ in U.MODE_SHAPES)
    for ws in U.WIDTH_CLASSES.values():  # every class has a width of every residue it can have
        assert {w % 4 for w in ws} >= ({1, 3} if len(ws) == 2 else {1, 2, 3})
    assert {64, 65, 66, 67, 95, 97} <= set(U.HEIGHTS) and max(U.HEIGHTS) <= 140
    assert U.HARRIS_BLOCK_ROWS - 1 in U.HEIGHTS and U.HARRIS_BLOCK_ROWS + 1 in U.HEIGHTS
    for rows in (U.NMS_BLOCK_ROWS, U.K_TH):  # a multiple, one below, one above
        rem = {h % rows for h in U.HEIGHTS}
        assert {0, 1, rows - 1} <= rem, rem
    assert max(w * h for w, h in U.ODD_SHAPES + U.MODE_SHAPES) <= 520 * 140
    for w, h, _ in U.ALIGNED_CASES:
        assert w % 4 == 0
    assert any(w > 256 for w, _ in U.MODE_SHAPES)


def test_stride_residues():
    assert [w * h % 4 for w, h in U.RESIDUE_SHAPES] == [1, 2, 3]
    assert set(U.stride_residues(65, 65)) == {0, 1, 2, 3} and set(U.stride_residues(67, 65)) == {0, 1, 2, 3}
    assert set(U.stride_residues(66, 65)) == {0, 2}
    per_residue = {r: 0 for r in range(4)}
    for w, h in U.ODD_SHAPES:
        for r in U.stride_residues(w, h):
            per_residue[r] += 1
    assert min(per_residue.values()) >= U.CENSUS_FLOOR, per_residue
    for w, h in U.RESIDUE_SHAPES:  # the flat image is not the only one at its residue
        assert U.stride_residues(w, h)[U.FLAT] in [r for i, r in enumerate(U.stride_residues(w, h)) if i != U.FLAT]


def test_every_case_takes_the_selection_form_it_is_filed_under():
    seen = set()
    for w, h in U.ODD_SHAPES:
        for form in U.FORMS:
            radius, maxk = U.form_params(form, w, h)
            assert select_form(w, h, radius, maxk) == form, (w, h, form, radius, maxk)
            seen.add(form)
    assert seen == set(U.FORMS)  # all three are reached at <= 520 x 140
    for w, h, form in U.ALIGNED_CASES:
        assert select_form(w, h, *U.form_params(form, w, h)) == form, (w, h, form)
    assert {f for _, _, f in U.ALIGNED_CASES} == {"array", "list"}
    for w, h in U.MODE_SHAPES:
        assert select_form(w, h, *U.form_params("array", w, h)) == "array"
    c = U.CAPACITY_CASE
    assert select_form(c["w"], c["h"], *U.form_params(c["form"], c["w"], c["h"])) == c["form"]
    assert select_form(259, 136, U.AGAST_TIE_RADIUS, U.AGAST_TIE_MAX_KPTS) == "grid"


def test_every_describe_case_takes_a_dense_route():
    # odd widths: whatever the pointer
    for w, h in U.ODD_SHAPES + U.MODE_SHAPES:
        for aligned in (False, True):
            assert describe_route(w, h, aligned, aware=False) in DENSE_ROUTES
            assert describe_route(w, h, aligned, aware=False, scale_invariant=True) == "kAllModes"
    for w, h in U.MODE_SHAPES:
        for model in ("radtan", "equidistant", "radtan8"):
            jac = U.camera_maps(w, h, model)[1]
            for aligned in (False, True):
                assert describe_route(w, h, aligned, True, jac=jac, fu=U.camera(w, h, model).fu) == "kAllModes"
    # aligned widths: the fast kernels at an aligned pointer, a dense route at offsets 1 .. 3
    for w, h, _ in U.ALIGNED_CASES:
        jac = U.camera_maps(w, h, U.ALIGNED_CAMERA)[1]
        fu = U.camera(w, h, U.ALIGNED_CAMERA).fu
        assert describe_route(w, h, True, aware=False) == "kRot"
        assert describe_route(w, h, True, aware=True, jac=jac, fu=fu) == "kAwareBatched"
        assert describe_route(w, h, False, aware=False) in DENSE_ROUTES
        assert describe_route(w, h, False, aware=True, jac=jac, fu=fu) in DENSE_ROUTES
    # the directed scenes of describe_scenes.py: every route, once its image batch is off the dword grid
    for name, r in DS.ROUTES.items():
        w = r.get("w", DS.W)
        jac = DS.fields(r["pattern"], w, DS.H)[0].jac
        kw = dict(pattern_key=r["pattern"], jac=jac, scale_invariant=r.get("scale_invariant", False),
                  steer=r.get("steer", 0.0))
        assert describe_route(w, DS.H, True, r["aware"], **kw) == r["expect"], name
        got = describe_route(w, DS.H, False, r["aware"], **kw)
        assert got in DENSE_ROUTES, (name, got)
        assert got not in ("kAwareBatched", "kRot", "kAware5", "kAware6", "kAwareWideBoxes")


def test_census_floors():
    c = U.census()
    short = {k: v for k, v in c.items() if v < U.CENSUS_FLOOR}
    assert not short, (short, c)


def test_candidate_capacity_of_the_cases():
    most = max(len(c) for w, h in U.ODD_SHAPES + U.MODE_SHAPES for c in U.candidates(w, h, U.THRESHOLDS[0]))
    assert most < U.MAX_CAND
    c = U.CAPACITY_CASE
    counts = [len(k) for k in U.candidates(c["w"], c["h"], c["thr"])]
    assert max(counts) > c["max_candidates"] and counts[U.FLAT] == 0
    # the two thresholds differ: dense and few
    for w, h in U.ODD_SHAPES:
        lo = sum(len(k) for k in U.candidates(w, h, U.THRESHOLDS[0]))
        hi = sum(len(k) for k in U.candidates(w, h, U.THRESHOLDS[1]))
        assert 0 < hi * 2 < lo, (w, h, lo, hi)
        assert len(U.candidates(w, h, U.THRESHOLDS[0])[U.FLAT]) == 0


def test_scale_space_layer_widths_cover_every_residue(oracle):
    residues = set()
    for w, h, octaves in U.SCALE_SPACE:
        for layer in range(2 * octaves):
            lw, lh = oracle.layer_size(w, h, layer)
            residues.add(lw % 4)
            assert lw * lh <= 520 * 140
    assert residues == {0, 1, 2, 3}, residues
    assert {o for _, _, o in U.SCALE_SPACE} == {1, 2}


def _selected(oracle, cand, w, h, radius, maxk):
    return oracle.uniformity_select(np.ascontiguousarray(cand), w, h, radius, maxk)


@pytest.mark.parametrize("form", ["array", "list"])
def test_a_wrong_score_or_a_missing_rim_candidate_shows_in_the_oracles_output(oracle, form):
    """What a kernel that is wrong at the rim would hand to the selection: the candidate list without one rim
    candidate (nms_generic_kernel's x < w - 2, harris_generic_kernel's column masks zeroing a maximum), or with one
    candidate's score one lower.  Per rim category, the number of candidates whose loss / change alters the kept set
    (position, score or order) must reach the floor over the scenes: the comparison against oracle.detect sees them."""
    seen = dict(col_2=0, col_w_minus_3=0, row_2=0, row_h_minus_3=0, partial_quad=0, score=0)
    for w, h in U.ODD_SHAPES:
        radius, maxk = U.form_params(form, w, h)
        for cand in U.candidates(w, h, U.THRESHOLDS[1]):
            if len(cand) == 0:
                continue
            want = _selected(oracle, cand, w, h, radius, maxk)
            rim = {"col_2": cand["x"] == 2, "col_w_minus_3": cand["x"] == w - 3, "row_2": cand["y"] == 2,
                   "row_h_minus_3": cand["y"] == h - 3, "partial_quad": (cand["x"] == w - 3) & (w % 4 == 3)}
            for name, mask in rim.items():
                for i in np.flatnonzero(mask)[:3]:
                    got = _selected(oracle, np.delete(cand, i), w, h, radius, maxk)
                    seen[name] += int(got.tobytes() != want.tobytes())
            for i in np.flatnonzero(rim["col_w_minus_3"] | rim["row_h_minus_3"])[:3]:
                off = cand.copy()
                off["score"][i] -= 1
                seen["score"] += int(_selected(oracle, off, w, h, radius, maxk).tobytes() != want.tobytes())
    assert min(seen.values()) >= U.CENSUS_FLOOR, seen


def test_agast_tie_scene_census(oracle):
    total = dict(crossing_255_256=0, starting_at_256_or_beyond=0, length_3_or_more=0)
    for w in U.AGAST_TIE_WIDTHS:
        score, cand, kps = U.agast_tie_reference(w)
        c = U.tie_run_census(score, U.AGAST_TIE_THR)
        for k in total:
            total[k] += c[k]
        assert len(cand) == len(kps) < U.AGAST_TIE_MAX_KPTS  # nothing suppressed: the kept set IS the accepted set
        assert int(U.passing_mask(score, U.AGAST_TIE_THR).sum()) > len(cand)  # the raster rule dropped some
        assert select_form(w, U.AGAST_TIE_HEIGHT, U.AGAST_TIE_RADIUS, U.AGAST_TIE_MAX_KPTS) == "grid"
    assert min(total.values()) >= U.CENSUS_FLOOR, total
    # per width: 333 has all three; 261 crosses into block 1's second lane; at 259 the last passing column is 255
    c261 = U.tie_run_census(U.agast_tie_reference(261)[0], U.AGAST_TIE_THR)
    c333 = U.tie_run_census(U.agast_tie_reference(333)[0], U.AGAST_TIE_THR)
    assert c261["crossing_255_256"] >= U.CENSUS_FLOOR and min(c333[k] for k in total) >= U.CENSUS_FLOOR
    p259 = U.passing_mask(U.agast_tie_reference(259)[0], U.AGAST_TIE_THR)
    assert int(p259[:, 255].sum()) >= U.CENSUS_FLOOR and not p259[:, 256:].any()

"""CPU: every entry point of include/okvfe.h that takes a context is classified for the pipelined-lanes contract
(okvfe_set_internal_lanes(ctx, -k)).  Lane work of a pipelined call is not ordered behind the caller's stream, so an
entry point that queues work touching the context's buffers must make its stream wait for the lanes (pick_stream), or
synchronise them on the host (lanes_join_host), or go through another entry point that does.  Anything else sits in
ALLOWED below with the reason it needs no join.  A new entry point fails here until someone has classified it.

A plain regex scan, not a parser: declarations end in ';', definitions are `okvfe_name(...) {` in csrc/*.cpp."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "okvfe.h")
SOURCES = sorted(glob.glob(os.path.join(ROOT, "okvis2_amd", "csrc", "*.cpp")))

JOIN_CALLS = ("pick_stream", "lanes_join_host")
# internal helpers that join on every path (their bodies are checked too)
JOINING_HELPERS = {"find_overflow": "lanes_join_host before it reads the candidate counts"}

HOST_MATCHER = "caller's host arrays in and out through scratch on the context's own stream; reads nothing the lanes write"
ALLOWED = {
    "okvfe_create": "makes the context: nothing is queued yet",
    "okvfe_destroy": "synchronises every stream of the context (join stream and lanes included) itself",
    "okvfe_last_error": "host-only: the error string",
    "okvfe_score_column": "host-only arithmetic on the live layout",
    "okvfe_set_keep_score_map": "host-only flag read by later calls",
    "okvfe_set_fp64_reduction": "synchronises the whole device before it writes the flag",
    "okvfe_get_pattern": "host-only copy of the installed pattern",
    "okvfe_pattern_kernel_class": "host-only classification of the installed pattern",
    "okvfe_gather_block_bytes": "host-only arithmetic",
    "okvfe_match_stereo": HOST_MATCHER,
    "okvfe_match_motion_stereo": HOST_MATCHER,
    "okvfe_match_motion_stereo_ext": HOST_MATCHER,
    "okvfe_match_to_map": HOST_MATCHER,
    "okvfe_match_to_map_landmarks": HOST_MATCHER + " (camera slots change only after a drain)",
    "okvfe_match_to_map_uninitialised": HOST_MATCHER,
    "okvfe_hamming_candidates": HOST_MATCHER,
    "okvfe_hamming_argmin": HOST_MATCHER,
    "okvfe_verify_place_match": HOST_MATCHER,
    "okvfe_fbrisk_transform": HOST_MATCHER,
    "okvfe_bow_query_l1": HOST_MATCHER,
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def ctx_entry_points():
    text = _strip_comments(open(HEADER).read())
    names = []
    for m in re.finditer(r"\b(okvfe_\w+)\s*\(([^;{}()]*(?:\([^()]*\)[^;{}()]*)*)\)\s*;", text):
        if re.search(r"\bokvfe_ctx\b", m.group(2)) and m.group(1) not in names:
            names.append(m.group(1))
    return names


def _bodies():
    bodies = {}
    for path in SOURCES:
        text = _strip_comments(open(path).read())
        for m in re.finditer(r"^[A-Za-z_][\w\s\*:<>,\"]*?\b(\w+)\s*\([^;{}]*\)\s*\{", text, flags=re.M):
            depth, i = 1, m.end()
            while depth and i < len(text):
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
            bodies.setdefault(m.group(1), text[m.end():i])
    return bodies


def _calls(body, name):
    return re.search(r"\b%s\s*\(" % re.escape(name), body) is not None


def classify():
    """-> (joining entry points, missing bodies, unclassified entry points)"""
    entry, bodies = ctx_entry_points(), _bodies()
    missing = [n for n in entry if n not in bodies]
    direct = JOIN_CALLS + tuple(JOINING_HELPERS)
    joins = {n for n in entry if n in bodies and any(_calls(bodies[n], c) for c in direct)}
    grown = True
    while grown:  # entry points that forward to an audited one
        new = {n for n in entry if n in bodies and n not in joins and any(_calls(bodies[n], j) for j in joins)}
        joins |= new
        grown = bool(new)
    unclassified = [n for n in entry if n in bodies and n not in joins and n not in ALLOWED]
    return joins, missing, unclassified


def test_header_scan_finds_the_entry_points():
    entry = ctx_entry_points()
    assert len(entry) >= 50, entry
    for n in ("okvfe_detect", "okvfe_compute", "okvfe_lanes_join", "okvfe_set_camera_maps", "okvfe_download_image_result",
              "okvfe_match_to_map_blocks_device", "okvfe_set_pattern", "okvfe_destroy", "okvfe_create"):
        assert n in entry, n


def test_joining_helpers_join():
    bodies = _bodies()
    for h in JOINING_HELPERS:
        assert h in bodies and any(_calls(bodies[h], c) for c in JOIN_CALLS), h


def test_every_ctx_entry_point_joins_or_is_allowed():
    joins, missing, unclassified = classify()
    assert not missing, f"declared in okvfe.h, no definition found in csrc/*.cpp: {missing}"
    assert not unclassified, (
        f"entry points that neither join pipelined lanes (pick_stream / lanes_join_host / an audited entry point) nor "
        f"sit in ALLOWED with a reason: {unclassified}")


def test_allow_list_is_not_stale():
    joins, _, _ = classify()
    entry = set(ctx_entry_points())
    assert not set(ALLOWED) - entry, f"ALLOWED names no entry point of okvfe.h: {sorted(set(ALLOWED) - entry)}"
    assert not set(ALLOWED) & joins, f"ALLOWED entries that do join (drop them from the list): {sorted(set(ALLOWED) & joins)}"
    for n, why in ALLOWED.items():
        assert why.strip(), n


def test_the_entry_points_the_contract_names_join():
    """The readers and the B = 1 / reconfiguration paths the lanes can race with join directly (not through a helper
    that happens to join on some path)."""
    bodies = _bodies()
    direct = {
        "okvfe_detect": "pick_stream", "okvfe_compute": "pick_stream", "okvfe_lanes_join": "pick_stream",
        "okvfe_set_camera_maps": "lanes_join_host", "okvfe_set_pattern": "lanes_join_host",
        "okvfe_download_image_result": "lanes_join_host", "okvfe_get_device_outputs": "lanes_join_host",
        "okvfe_profile_read": "lanes_join_host", "okvfe_profile_enable": "lanes_join_host",
        "okvfe_set_internal_lanes": "lanes_join_host", "okvfe_pack_gather_blocks_device": "pick_stream",
        "okvfe_match_stereo_blocks_batch_device": "pick_stream", "okvfe_match_to_map_blocks_device": "pick_stream",
    }
    for n, c in direct.items():
        assert n in bodies and _calls(bodies[n], c), (n, c)

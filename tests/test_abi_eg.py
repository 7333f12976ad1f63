"""The C ABI of the essential-graph optimisation (include/vsg_orb.h: vsg_mappoints_optimize_essential_graph and
vsg_mappoints_correct_sim3) without a device: the symbols, the signatures as the header, the kernel file, the binding and the
adaptor have them, the layout of vsg_essential_graph_result, the reference lines and the refusals the header cites, and the
argument errors that are decided before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import eg_hostcore as hc
import eg_scenes as es
from test_eg_hostmath import error_cases
from visual_sgraphs_amd import orb

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_eg"
NAME, CORRECT = "vsg_mappoints_optimize_essential_graph", "vsg_mappoints_correct_sim3"
INVALID, UNSUPPORTED, NO_DEVICE = -6, -3, -4


def _declaration(text, name):
    m = re.search(r"\bint %s\((.*?)\)\s*[;{]" % name, text, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def _header_comment(before):
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    end = header.index(before)
    return re.sub(r"\s*\n \*\s*", " ", header[header.rindex("/*", 0, end):end])


def test_symbols_are_exported_declared_and_bound():
    L = orb.load_library()
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    kernel = (ROOT / "visual_sgraphs_amd" / "csrc" / "vsg_essential_graph.hip").read_text()
    for name in (NAME, CORRECT):
        assert hasattr(L, name) and name in orb.EXPORTS
        assert _declaration(header, name) == _declaration(kernel, name)
    assert _declaration(header, NAME) == [
        "vsg_mappoints *mp", "int n_kf", "const vsg_sim3d *kf_Scw", "const vsg_sim3d *kf_non_corrected",
        "const uint8_t *kf_has_non_corrected", "const uint8_t *kf_fixed", "int n_edges", "const int32_t *edge_i",
        "const int32_t *edge_j", "const uint8_t *edge_loop", "int fix_scale", "int iterations", "int n_points",
        "const int32_t *slots", "const int32_t *point_ref", "vsg_sim3d *kf_Scw_out", "float *world_pos_out", "double *chi2",
        "vsg_essential_graph_result *res"]
    assert _declaration(header, CORRECT) == [
        "vsg_mappoints *mp", "int n_points", "const int32_t *slots", "const int32_t *point_ref", "int n_ref",
        "const vsg_sim3d *S_from", "const vsg_sim3d *S_to_inverse", "float *world_pos_out"]
    assert len(L.vsg_mappoints_optimize_essential_graph.argtypes) == 19 and len(L.vsg_mappoints_correct_sim3.argtypes) == 8
    assert "vsg_essential_graph.hip" in (ROOT / "visual_sgraphs_amd" / "build.py").read_text()


def test_header_cites_the_reference_and_lists_every_refusal():
    text = _header_comment("typedef struct vsg_essential_graph_result")
    for cite in ("Optimizer.cc:2456-2734", "LoopClosing.cc:1150", ":2469", ":2684", ":2502-2511", ":2514", ":2529-2560", ":2563-2660",
                 ":2712-2721", ":2723-2728", ":2700", ":2662-2679", ":2736"):
        assert cite in text, cite
    for refusal in ("a negative count", "a NULL kf_Scw_out or res", "a NULL kf_Scw, kf_has_non_corrected or kf_fixed",
                    "a NULL kf_non_corrected with an entry flagged", "a NULL edge_i, edge_j or edge_loop", "a NULL mp, slots or point_ref",
                    "fix_scale outside {0, 1}", "iterations outside [1, 100]", "an edge index outside [0, n_kf)",
                    "edge_i[e] == edge_j[e]", "a slot outside [0, capacity), or listed twice", "a point_ref outside [0, n_kf)",
                    "not finite or whose scale is <= 0", "more than 438 keyframes", "an error writes nothing"):
        assert refusal in text, refusal
    assert orb.ESSENTIAL_GRAPH_MAX_OPT_KF == 438 and 7 * 438 <= 3072 < 7 * 439
    text = _header_comment("int vsg_mappoints_correct_sim3(")
    for cite in ("LoopClosing.cc:1060-1064", "Optimizer.cc:2723-2728", "an error writes nothing", "listed twice", "a point_ref outside [0, n_ref)"):
        assert cite in text, cite


def test_every_refusal_of_the_header_is_a_case_of_the_tests():
    _, cases = error_cases()
    for case in ("null_Scw", "null_has", "null_fixed", "null_nonc_with_entry", "null_edge_i", "null_edge_j", "null_edge_loop", "null_slots",
                 "null_point_ref", "null_store_with_points", "null_kf_out", "null_res", "negative_n_kf", "negative_n_edges",
                 "negative_n_points", "edge_i_negative", "edge_i_past_end", "edge_j_negative", "edge_j_past_end", "edge_self",
                 "slot_negative", "slot_past_end", "slot_twice", "ref_negative", "ref_past_end", "Scw_nan", "Scw_inf", "Scw_scale_zero",
                 "Scw_scale_negative", "nonc_nan_on_entry", "nonc_scale_zero_on_entry", "fix_scale_2", "iterations_0", "iterations_101"):
        assert case in cases, case
    assert {c for _, c in cases.values()} == {INVALID}  # VSG_ERR_UNSUPPORTED is test_cap_is_438_optimised_keyframes


def test_result_layout_matches_the_header(tmp_path):
    header = (ROOT / "include" / "vsg_orb.h").read_text()
    m = re.search(r"typedef struct vsg_essential_graph_result \{(.*?)\} vsg_essential_graph_result;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for part in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in part.split(",")]
    assert tuple(names) == hc.RESULT_INTS + hc.RESULT_DOUBLES == orb.ESSENTIAL_GRAPH_RESULT_INTS + orb.ESSENTIAL_GRAPH_RESULT_DOUBLES
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vsg_orb.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vsg_essential_graph_result));\n' +
                   "".join('  printf(" %%zu", offsetof(vsg_essential_graph_result, %s));\n' % f for f in names) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    for R in (orb.EssentialGraphResult, hc.Result):
        assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in names]
    assert got == [64] + [4 * i for i in range(10)] + [40, 48, 56]


def test_cpp_adaptor_compiles_and_fails_loudly_without_device():
    L = orb.load_library()
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    adaptor = (ROOT / "include" / "vsg_orb_adaptor.hpp").read_text()
    for name in ("EssentialGraphResult OptimizeEssentialGraph(", "struct EssentialGraphResult", "struct EssentialGraphEdges",
                 "inline EssentialGraphEdges essential_graph_edges(", "std::vector<float> CorrectSim3(", NAME + "(", CORRECT + "(",
                 "bFixScale", ":2542", ":2608", ":2634-2639"):
        assert name in adaptor, name
    m = re.search(r"check\(%s\((.*?)\),\s*\"%s\"\)" % (NAME, NAME), adaptor, re.S)
    assert m and len(re.sub(r"\([^()]*\)", "", m.group(1)).split(",")) == 19  # the header's nineteen arguments
    if L.vsg_device_count() <= 0:
        r = subprocess.run([str(ADAPTOR / "eg_check"), "/dev/null", "/dev/null"], capture_output=True, text=True)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout


def _raw(L, s, mp=None, null=(), **over):
    s = dict(s, **over)
    a = hc.marshal(s)
    K, E, P = a["Scw"].shape[0], a["ei"].size, a["slots"].size
    kf_out, pos_out, chi2 = np.full((max(K, 1), 8), hc.SENT), np.full((max(P, 1), 3), hc.SENT, np.float32), np.full(max(E, 1), hc.SENT)
    res = orb.EssentialGraphResult()
    res.ran = -77
    ip, fp, bp, dp, sp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(orb.Sim3d)
    arg = lambda name, v, t: None if name in null else C.cast(v.ctypes.data_as(C.c_void_p), t)
    rc = L.vsg_mappoints_optimize_essential_graph(
        mp, K, arg("Scw", a["Scw"], sp), arg("nonc", a["nonc"], sp), arg("has", a["has"], bp), arg("fixed", a["fixed"], bp), E,
        arg("ei", a["ei"], ip), arg("ej", a["ej"], ip), arg("el", a["el"], bp), int(s["fix_scale"]), int(s["iterations"]), P,
        arg("slots", a["slots"], ip), arg("ref", a["ref"], ip), arg("kf_out", kf_out, sp), arg("pos_out", pos_out, fp),
        arg("chi2", chi2, dp), None if "res" in null else C.byref(res))
    untouched = (kf_out == hc.SENT).all() and (pos_out == hc.SENT).all() and (chi2 == hc.SENT).all() and res.ran == -77
    return rc, untouched, kf_out[:K], res


def test_argument_errors_need_no_device():
    """What the library decides before it looks for a device: with a NULL store every check of the pose graph's own
    arguments, and the points' need of a store."""
    L = orb.load_library()
    base, cases = error_cases()
    none = dict(slots=np.zeros(0, np.int32), point_ref=np.zeros(0, np.int32))
    assert _raw(L, base)[:2] == (INVALID, True)  # points without a store
    for case, (kw, code) in sorted(cases.items()):
        if any(k in kw for k in ("slots", "point_ref", "n_kf", "n_edges", "n_points")) or \
                any(n in kw.get("null", ()) for n in ("slots", "ref", "store")):
            continue  # the points' checks need a store
        over = {k: v for k, v in kw.items() if k != "null"}
        rc, untouched, _, _ = _raw(L, base, null=kw.get("null", ()), **dict(none, **over))
        assert (rc, untouched) == (code, True), case
    assert L.vsg_mappoints_correct_sim3(None, 0, None, None, 0, None, None, None) == INVALID


def test_nothing_to_optimise_needs_no_device():
    """res->ran = 0 is decided before a device is looked for: no edge, and edges between fixed keyframes alone."""
    L = orb.load_library()
    base = es.scenes()["loop_fix0_s1"]
    none = dict(slots=np.zeros(0, np.int32), point_ref=np.zeros(0, np.int32))
    for over in (dict(ei=np.zeros(0, np.int32), ej=np.zeros(0, np.int32), eloop=np.zeros(0, np.uint8)),
                 dict(fixed=np.ones(len(base["fixed"]), np.uint8))):
        rc, _, kf_out, res = _raw(L, base, **dict(none, **over))
        assert rc == 0 and res.ran == 0 and res.n_opt_kf == 0 and res.trials_run == 0
        assert kf_out.tobytes() == np.asarray(base["Scw"], np.float64).tobytes()
    if L.vsg_device_count() <= 0:  # a real problem then fails loudly: there is no CPU path in the library
        assert _raw(L, base, **none)[0] in (NO_DEVICE, -5)

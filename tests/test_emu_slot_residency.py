"""What every slot holds after every call that changes it (the transition table above `struct Residency` in csrc/mot_host.h), walked on
the emulator build in two-step pairs: a fused batch over slots 0 and 1, then ONE call that changes what slot 0 holds, then ONE getter on
slot 0 or on slot 1 (the other slot of the earlier batch) — a fresh context per cell, since a getter may itself materialise something.

Each cell of TABLE is what the getter must answer:
    EQ          MOT_OK and data equal to the oracle's for the cloud now resident in the slot
    OLD         MOT_OK and the box stage's results of the slot's PREVIOUS cloud, untouched (mot_get_boxes is not vouched for after a stage-wise call
                that ran no box stage: include/mot.h; mot_box_markers is what refuses)
    ANY         MOT_OK, content not vouched for (label grid of one cloud, points of another)
    a code      the call is refused with it
The codes, OLD and ANY were recorded from the library as it was BEFORE slot residency got one owner (they are not derived from the code under test)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

N, STRIDE, B = 3000, 3072, 2
EQ, OLD, ANY = "EQ", "OLD", "ANY"
STATE = 4    # MOT_E_STATE (held against the package's constant in `world`)

GETTERS = ("elevated", "ground", "mask", "labels", "boxes", "markers", "products")
TRANSITIONS = ("fused_0", "fused_labels", "fused_ground", "fused_ground_mask", "ground_remove", "ground_node_frame", "ground_remove_pointcloud2",
               "cluster_labels", "cluster_no_labels", "box_fit", "box_fit_resident", "cluster_products_host", "cluster_node_frame")

# TABLE[transition] = (slot 0's row, slot 1's row), one entry per getter in GETTERS order
TABLE = {
    'fused_0': ((EQ, EQ, EQ, EQ, EQ, EQ, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'fused_labels': ((EQ, EQ, EQ, EQ, EQ, EQ, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'fused_ground': ((EQ, EQ, EQ, EQ, EQ, EQ, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'fused_ground_mask': ((EQ, EQ, EQ, EQ, EQ, EQ, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'ground_remove': ((EQ, EQ, EQ, ANY, OLD, STATE, ANY), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'ground_node_frame': ((EQ, STATE, STATE, ANY, OLD, STATE, ANY), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'ground_remove_pointcloud2': ((EQ, EQ, EQ, ANY, OLD, STATE, ANY), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'cluster_labels': ((STATE, STATE, STATE, EQ, OLD, STATE, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'cluster_no_labels': ((STATE, STATE, STATE, EQ, OLD, STATE, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'box_fit': ((STATE, STATE, STATE, EQ, EQ, EQ, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
    'box_fit_resident': ((EQ, EQ, EQ, EQ, EQ, EQ, EQ), (EQ, EQ, EQ, EQ, EQ, EQ, EQ)),
    'cluster_products_host': ((STATE, STATE, STATE, ANY, OLD, STATE, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),   # labels, slot 0: see test_products_host_invalidates_the_previous_labels
    'cluster_node_frame': ((STATE, STATE, STATE, EQ, EQ, EQ, EQ), (STATE, STATE, STATE, EQ, EQ, EQ, EQ)),
}


@pytest.fixture(scope="module")
def emu(mot):
    import build_emu
    lib = build_emu.build()
    return lib, mot.load_library(lib)


@pytest.fixture(scope="module")
def world(mot, synth, _oracle_module):
    """the clouds of the walk and the oracle's answers for each of them"""
    O = _oracle_module
    assert STATE == mot.MOT_E_STATE
    p = O.params(0)

    def answers(elev, g=None):
        cl = O.cluster(p, elev)
        bx = O.box_fit(p, elev, cl["grid"], cl["num_cluster"])
        return dict(elevated=elev, ground=g["ground"] if g else None, mask=g["mask"] if g else None, grid=cl["grid"], num_cluster=cl["num_cluster"],
                    labels=cl["point_label"], boxes=bx["boxes"], markers=O.box_markers_numpy(elev, cl["point_label"], bx["box_cluster"]),
                    products=O.cluster_products(p, elev, cl["grid"]))

    def from_raw(raw):
        g = O.ground_remove(p, raw)
        return answers(g["elevated"], g)

    clouds = {}
    for name, seed in (("F0", 11), ("F1", 12), ("G0", 13), ("R", 14), ("S", 15)):
        a = synth.make_cloud(N, seed, seed % 3).astype(np.float32)
        a[:, 3] = 1.0   # (the PointCloud2 entry point writes 1.0f for the 4th value: the same oracle answer serves the three ground calls)
        clouds[name] = np.ascontiguousarray(a)
    w = {k: from_raw(clouds[k]) for k in ("F0", "F1", "G0", "R")}
    A = np.ascontiguousarray(O.ground_remove(p, clouds["S"])["elevated"][::-1])   # the cloud of the stage-wise cluster / box calls
    w["A"] = answers(A)
    host = np.zeros((B, STRIDE, 4), np.float32)
    host[0, :N] = clouds["F0"]; host[1, :N] = clouds["F1"]
    one = np.zeros((1, STRIDE, 4), np.float32); one[0, :N] = clouds["G0"]
    return dict(raw=clouds, ans=w, host=host, one=one, A=A)


def _transition(mot, c, L, w, name):
    """runs the call; returns the key of the cloud that slot 0 holds afterwards"""
    A, a = w["A"], w["ans"]["A"]
    if name.startswith("fused_"):
        c.set_fused_outputs({"0": 0, "labels": mot.OUT_LABELS, "ground": mot.OUT_GROUND, "ground_mask": mot.OUT_GROUND | mot.OUT_MASK}[name[6:]])
        c.frames_dev(w["one"].ctypes.data, STRIDE * 4, [N])   # a batch of ONE: slot 1 is then a slot beyond the last batch
        return "G0"
    if name == "ground_remove":
        c.ground_remove(w["raw"]["R"]); return "R"
    if name == "ground_node_frame":
        c.ground_node_frame(w["raw"]["R"]); return "R"
    if name == "ground_remove_pointcloud2":
        c.ground_remove_pointcloud2(w["raw"]["R"].view(np.uint8).reshape(-1), N, 16, 0, 4, 8); return "R"
    if name == "cluster_labels":
        c.cluster(A); return "A"
    if name == "cluster_no_labels":
        grid = np.zeros_like(a["grid"]); nc = C.c_int(0)
        assert L.mot_cluster(c._h, A.ctypes.data_as(C.c_void_p), len(A), grid.ctypes.data_as(C.c_void_p), C.byref(nc), None) == 0
        return "A"
    if name == "box_fit":
        c.box_fit(A, a["grid"], a["num_cluster"]); return "A"
    if name == "box_fit_resident":
        c.box_fit_resident(); return "F0"
    if name == "cluster_products_host":
        c.cluster_products_host(A, a["grid"]); return "A"
    assert name == "cluster_node_frame"
    c.cluster_node_frame(A); return "A"


def _get(c, L, slot, getter):
    """(return code, data) of one getter asking for one thing"""
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    if getter in ("elevated", "ground", "mask"):
        buf = np.zeros(STRIDE, np.uint8) if getter == "mask" else np.zeros((STRIDE, 4), np.float32)
        ne, ng = C.c_int(0), C.c_int(0)
        rc = L.mot_get_ground(c._h, slot, vp(buf) if getter == "elevated" else None, C.byref(ne), vp(buf) if getter == "ground" else None, C.byref(ng),
                              vp(buf) if getter == "mask" else None, STRIDE)
        return rc, buf[: {"elevated": ne.value, "ground": ng.value, "mask": N}[getter]]
    if getter == "labels":
        G = c.params.num_grid
        grid = np.zeros((G, G), np.int32); nc = C.c_int(0); lab = np.full(STRIDE, -7, np.int32)
        rc = L.mot_get_clusters(c._h, slot, vp(grid), C.byref(nc), vp(lab), STRIDE)
        return rc, (grid, lab)
    try:
        if getter == "boxes":
            return 0, c.get_boxes(slot)["boxes"]
        if getter == "markers":
            return 0, c.box_markers(slot)
        return 0, c.cluster_products(slot)
    except Exception as e:   # mot.MotError
        return e.code, None


def _same(getter, data, want):
    if getter == "labels":
        n = len(want["labels"])
        return np.array_equal(data[0], want["grid"]) and np.array_equal(data[1][:n], want["labels"])
    if getter == "products":
        return all(np.array_equal(data[k], want["products"][k]) for k in ("clustered", "obstacles", "cost_map"))
    if want[getter] is None:
        return False
    a, b = np.asarray(data), np.asarray(want[getter])
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def outcome(mot, emu, w, transition, slot, getter):
    lib, L = emu
    with mot.Context(lib_path=lib, max_points=STRIDE, max_batch=B, max_tracks_total=16) as c:
        c.frames_dev(w["host"].ctypes.data, STRIDE * 4, [N] * B)
        held = _transition(mot, c, L, w, transition) if slot == 0 else (_transition(mot, c, L, w, transition), "F1")[1]
        rc, data = _get(c, L, slot, getter)
    if rc != 0:
        return rc
    if _same(getter, data, w["ans"][held]):
        return EQ
    if slot == 0 and _same(getter, data, w["ans"]["F0"]):
        return OLD
    return ANY


@pytest.mark.parametrize("transition", TRANSITIONS)
def test_transition_table(mot, emu, world, transition):
    got = tuple(tuple(outcome(mot, emu, world, transition, slot, g) for g in GETTERS) for slot in (0, 1))
    assert got == TABLE[transition], (transition, dict(zip(GETTERS, zip(*got))))


def test_products_host_invalidates_the_previous_labels(mot, emu, world):
    """mot_cluster(A, labels) then mot_cluster_products_host(B, grid of B): mot_get_clusters(0, point_label) must answer B's labels. FAILS on the
    library as it was before residency got one owner: alone among the calls that take slot 0, mot_cluster_products_host left the slot's label
    state untouched, and the getter handed back A's labels for B's points.
    (The cluster_products_host / labels / slot 0 cell of TABLE stays ANY all the same: the label kernel takes every label above the slot's cluster COUNT
    for "no cluster", and mot_cluster_products_host — which has no num_cluster argument — leaves the count of the slot's previous cloud, there the fused
    batch's 22 against 29 labels in the uploaded grid. Here A's count covers B's labels.)"""
    lib, L = emu
    A, a = world["A"], world["ans"]["A"]
    b = world["ans"]["F1"]; Bc = np.ascontiguousarray(b["elevated"])
    assert len(A) != len(Bc) or not np.array_equal(a["labels"], b["labels"])
    with mot.Context(lib_path=lib, max_points=STRIDE, max_batch=1, max_tracks_total=16) as c:
        assert np.array_equal(c.cluster(A)["point_label"], a["labels"])
        c.cluster_products_host(Bc, b["grid"])
        got = c.get_clusters(0, n_elevated=len(Bc))
        assert np.array_equal(got["grid"], b["grid"]) and np.array_equal(got["point_label"], b["labels"])

"""The per-frame capacity edges of the cluster and box stage (tests/capacity_cases.py) on the emulator: at each limit bit-exact against
the oracle, one beyond it refused — by kernels that stay inside their buffers (run this file under MOT_EMU_SANITIZE=address before the
GPU file goes anywhere: tests/README.md) — and the contract after a refusal. Plus the limits no input reaches, as computed bounds."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "csrc")


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("max_points,permuted", [(8192, False), (12288, True), (16384, False)])
def test_emu_group_edge_stagewise(env, oracle, max_points, permuted):
    """12288 with the permuted cloud is the reported crash (segmentation fault inside mot_box_fit before the fix)"""
    CC.groups_stagewise(env, oracle, max_points, permuted)


def test_emu_refused_frame_finds_nothing_of_an_earlier_frame(env, oracle):
    CC.groups_refused_first(env, oracle)


def test_emu_cluster_edge_stagewise(env, oracle):
    CC.clusters_stagewise(env, oracle)


def test_emu_box_edge_stagewise(env, oracle):
    CC.boxes_stagewise(env, oracle)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("kind", ["groups", "clusters", "boxes"])
def test_emu_fused_refusal_contract(env, oracle, kind, graphs):
    CC.fused_contract(env, oracle, kind, graphs)


def test_emu_sequence_mode_reports_a_refused_frame(env, oracle):
    CC.sequence_refusal(env, oracle)


def test_preset0_cannot_reach_the_cluster_limit(oracle):
    CC.preset0_cluster_ceiling(oracle)


def test_emu_ram_points_edge(env, oracle):
    CC.ram_points_edge(env, oracle)


def test_hull_limit_is_out_of_reach():
    """kMaxHull against a computed bound. A cluster's picture lies in 901 x 901 pixels at the presets (box.hip: kMaxHullIn = 2 * 901): a span of 900
    steps (bound 328); in 1001 x 1001 pixels at the largest pic_scale * roi_m mot_create admits (bound 352).
    The bound counts STRICTLY convex polygons; the hull code must therefore drop collinear points — peel_chain keeps a point only on a strict
    turn (`cr < 0` / `cr > 0`), which is checked here against the source as well."""
    src = open(os.path.join(CSRC, "box.hip")).read()
    k_max_hull = int(re.search(r"constexpr int kMaxHull = (\d+);", src).group(1))
    assert int(re.search(r"constexpr int kMaxHullIn = 2 \* (\d+);", src).group(1)) == 901
    assert re.search(r"keep = sign > 0 \? \(cr < 0\) : \(cr > 0\);", src), "peel_chain no longer drops collinear points: the bound below does not hold"
    bound = CC.lattice_polygon_vertex_bound(900)
    print("vertex bound of a convex lattice polygon in 901 x 901 pixels:", bound)
    assert 300 < bound <= k_max_hull
    # mot_create admits pic_scale * roi_m up to 1000: a picture of 1001 x 1001 pixels, a span of 1000 steps
    wide = CC.lattice_polygon_vertex_bound(1000)
    print("vertex bound of a convex lattice polygon in 1001 x 1001 pixels:", wide)
    assert bound <= wide <= k_max_hull
    assert [CC.lattice_polygon_vertex_bound(s) for s in (1, 2, 3)] == [4, 6, 8]   # tight where it can be checked by hand: unit square, hexagon, octagon
